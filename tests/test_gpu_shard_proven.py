"""The proven-complaint rule on dealer shards: dkg_ceremony_shard_verify_proven_device /
_shard_verify_full_proven_device per rank, dkg_shard_combine_proven_device on the gathered blocks.

Ranks are emulated on one GPU, one Backend per rank, and driven as a multi-rank driver drives them
(run_sharded: shard call, pack, "gather" into one buffer, combine, reconstruction on the owning ranks,
finalise).  The reference of every assertion is the single-context call on the same inputs
(ceremony_verify_full_proven / ceremony_verify_fetched_proven), which the libsodium fixtures and the
oracle pin; one case also checks the merged verdicts against the oracle directly, and the combine
against the Python model of tests/test_shard_proven.py.
"""
import ctypes
import dataclasses
import random

import pytest

import dkg_amd
from dkg_amd import (COMPLAINT_IGNORED, COMPLAINT_NO_PHASE3, COMPLAINT_NOT_OWNED, MISSING, REJECT, SELF, _lib,
                     merge_verdicts, packed_row_words, shard_range, shard_rows)
from dkg_amd._lib import DKG_E_ARG, DKG_OK, FIN_INSUFFICIENT, FIN_OK, FIN_PANIC, FIN_PHASE4_ERROR
from tests import oracle_lib as O
from tests.test_gpu import CK
from tests.test_gpu_batch_proven import bump, faulted_ceremony, golden_full, oracle2, oracle4, pair, sc
from tests.test_gpu_complaints import enc_of
from tests.test_shard_proven import FLAG_NO_PHASE3, FLAG_ROUND2, FLAG_ROUND4, flag_outcome

pytestmark = pytest.mark.gpu

H = bytes.fromhex
ZERO = bytes(32)


@pytest.fixture(scope="module")
def be():
    b = dkg_amd.Backend(0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def ranks():
    """One context per emulated rank (each remembers its own shard's decrypted shares)."""
    bs = [dkg_amd.Backend(0) for _ in range(3)]
    yield bs
    for b in bs:
        b.close()


def _dev(x):
    import torch

    return torch.frombuffer(bytearray(x or bytes(16)), dtype=torch.uint8).to("cuda:0")


def _host(t):
    return bytes(t.cpu().numpy())


@dataclasses.dataclass
class Sharded:
    fields: tuple        # what _fields gives for the single-context result
    verdict: list        # merged over the ranks
    verdict4: list
    dissent: list
    finalise_status: int
    recovery_index: int
    flags: list          # [n], compacted
    per_rank: list       # (verdict, verdict4) of each rank
    evals: list          # last_complaint_eval of each rank
    reruns: list         # binomial_reruns of each rank
    model: dict          # tests/test_shard_proven.flag_outcome on the ranks' raw rows and flags


def _fields(r):
    """The comparable outputs of a single-context CeremonyResult."""
    return (bytes(r.dec2), bytes(r.dec4), list(r.qualified), list(r.r2_error), list(r.complaints2), list(r.reconstruct),
            list(r.r4_error), int(r.phase4_error), r.n_qualified, r.final_share, r.public_share, r.mpk)


def lists2(c2):
    return [x[0] for x in c2], [x[1] for x in c2], b"".join(x[2] for x in c2)


def lists4(c4):
    return [x[0] for x in c4], [x[1] for x in c4], b"".join(x[2] for x in c4), b"".join(x[3] for x in c4)


def run_sharded(ranks, ws, cer, c2, c4, full=True, f1=None, f3=None):
    """The ceremony `cer` (host arrays E, A and e1 / ct / sk / pk or s / s_prime) over ws emulated ranks with
    the broadcast complaint lists c2 [(accuser, accused, proof)] and c4 [(accuser, accused, share,
    randomness)] passed WHOLE to every rank."""
    import torch

    n, t = cer["n"], cer["t"]
    N = t + 1
    R, W = shard_rows(n, ws), packed_row_words(n)
    i32, u8 = dict(dtype=torch.int32, device="cuda:0"), dict(dtype=torch.uint8, device="cuda:0")
    pack2, pack4 = torch.zeros(ws * R * W, **i32), torch.zeros(ws * R * W, **i32)
    flags = torch.full((ws * R,), -1, **i32)  # poisoned: the call writes every word of its block
    dissent = torch.full((ws * n,), -1 if full else 0, **i32)
    terms, partials = torch.zeros(ws * R * 32, **u8), torch.full((ws * n * 32,), 0xEE, **u8)
    raw2, raw4, per_rank, evals, reruns, keep = [], [], [], [], [], []
    for r in range(ws):
        b = ranks[r]
        b.env_init(t, n, CK)
        d0, d1 = shard_range(n, ws, r)
        D = d1 - d0
        o2, o4 = torch.zeros(max(D * n, 16), **u8), torch.zeros(max(D * n, 16), **u8)
        dE, dA = _dev(cer["E"][32 * N * d0:32 * N * d1]), _dev(cer["A"][32 * N * d0:32 * N * d1])
        m1 = None if f1 is None else bytes(f1[d0:d1])
        m3 = None if f3 is None else bytes(f3[d0:d1])
        out = (o2.data_ptr(), o4.data_ptr(), terms[32 * R * r:].data_ptr(), partials[32 * n * r:].data_ptr(), R,
               flags[R * r:].data_ptr())
        if full:
            x1, x2 = _dev(cer["e1"][64 * n * d0:64 * n * d1]), _dev(cer["ct"][64 * n * d0:64 * n * d1])
            _, v2, v4 = b.ceremony_shard_verify_full_proven_device(
                n, t, d0, d1, dE.data_ptr(), dA.data_ptr(), x1.data_ptr(), x2.data_ptr(), cer["sk"], cer["pk"],
                *lists2(c2), *lists4(c4), *out, dissent[n * r:].data_ptr(), fetched1=m1, fetched3=m3)
        else:
            x1, x2 = _dev(cer["s"][32 * n * d0:32 * n * d1]), _dev(cer["s_prime"][32 * n * d0:32 * n * d1])
            _, v4 = b.ceremony_shard_verify_proven_device(
                n, t, d0, d1, dE.data_ptr(), dA.data_ptr(), x1.data_ptr(), x2.data_ptr(), *lists4(c4), *out,
                fetched1=m1, fetched3=m3)
            v2 = []
        keep += [dE, dA, x1, x2]
        evals.append(b.last_complaint_eval())
        reruns.append(b.binomial_reruns())
        per_rank.append((v2, v4))
        # ownership: a verdict exactly for the complaints against this rank's dealers
        assert [v != COMPLAINT_NOT_OWNED for v in v4] == [d0 < x[1] <= d1 for x in c4], r
        assert [v != COMPLAINT_NOT_OWNED for v in v2] == [d0 < x[1] <= d1 for x in c2], r
        b.decisions_pack_device(R, D, n, d0, o2.data_ptr(), pack2[R * W * r:].data_ptr())
        b.decisions_pack_device(R, D, n, d0, o4.data_ptr(), pack4[R * W * r:].data_ptr())
        raw2 += [list(_host(o2)[n * i:n * i + n]) for i in range(D)]
        raw4 += [list(_host(o4)[n * i:n * i + n]) for i in range(D)]
    fl = flags.tolist()
    for r in range(ws):
        d0, d1 = shard_range(n, ws, r)
        assert fl[R * r + d1 - d0:R * (r + 1)] == [0] * (R - (d1 - d0)), "padding rows of the flag block"
    cd2, cd4 = torch.zeros(n * n, **u8), torch.zeros(n * n, **u8)
    c0 = ranks[0]
    o, dis, st, ri = c0.shard_combine_proven_device(n, t, ws, pack2.data_ptr(), pack4.data_ptr(), flags.data_ptr(),
                                                    dissent.data_ptr() if full else None, full, cd2.data_ptr(),
                                                    cd4.data_ptr())
    no_mpk = st in (FIN_PANIC, FIN_PHASE4_ERROR)
    assert (st == FIN_PHASE4_ERROR) == o.phase4_error
    if any(o.reconstruct) and not no_mpk:
        fails = set()
        for r in range(ws):
            d0, d1 = shard_range(n, ws, r)
            fails.add(ranks[r].ceremony_shard_recon_device(n, t, d0, d1, o.qualified, o.reconstruct, None,
                                                           terms[32 * R * r:].data_ptr(), o.r2_error, o.r4_error))
        assert len(fails) == 1  # decided from the common outcome: the same on every rank
        assert fails == {st == FIN_INSUFFICIENT}
        no_mpk = fails.pop()
    fs, pub = torch.zeros(32 * n, **u8), torch.zeros(32 * n, **u8)
    mpk = c0.shard_finalise_device(n, t, ws, terms.data_ptr(), partials.data_ptr(), o.qualified, no_mpk, fs.data_ptr(),
                                   pub.data_ptr())
    flat = [fl[R * r + i] for r in range(ws) for i in range(shard_range(n, ws, r)[1] - shard_range(n, ws, r)[0])]
    fields = (_host(cd2), _host(cd4), o.qualified, o.r2_error, o.complaints2, o.reconstruct, o.r4_error,
              int(o.phase4_error), o.n_qualified, _host(fs), _host(pub), mpk)
    return Sharded(fields, merge_verdicts([p[0] for p in per_rank]) if c2 else [],
                   merge_verdicts([p[1] for p in per_rank]) if c4 else [], dis, st, ri, flat, per_rank, evals, reruns,
                   flag_outcome(n, t, raw2, raw4, flat, full))


def single_full(be, cer, c2, c4, f3=None):
    be.env_init(cer["t"], cer["n"], CK)
    return be.ceremony_verify_full_proven(cer["E"], cer["A"], cer["e1"], cer["ct"], cer["sk"], cer["pk"], *lists2(c2),
                                          *lists4(c4), cer["n"], cer["t"], fetched3=f3)


def single_plain(be, cer, c4, f1=None, f3=None):
    n = cer["n"]
    be.env_init(cer["t"], n, CK)
    return be.ceremony_verify_fetched_proven(cer["E"], cer["A"], cer["s"], cer["s_prime"], f1 or bytes([1] * n),
                                             f3 or bytes([1] * n), *lists4(c4), n, cer["t"])


def assert_same(sh, p, full):
    assert sh.fields == _fields(p.result)
    assert sh.verdict4 == p.verdict4
    assert (sh.finalise_status, sh.recovery_index) == (p.finalise_status, p.recovery_index)
    if full:
        assert sh.verdict == p.verdict and sh.dissent == p.dissent
    m = sh.model  # the combine is what the flag-word model says
    f = sh.fields
    assert (f[2], f[3], f[4], f[5], f[6], f[7], f[8]) == (m["qualified"], m["r2_error"], m["complaints2"],
                                                          m["reconstruct"], m["r4_error"], m["phase4_error"],
                                                          m["n_qualified"])
    assert list(f[1]) == [x for row in m["dec4"] for x in row]
    assert (sh.finalise_status, sh.recovery_index) == (m["finalise_status"], m["recovery_index"])


# ---------------------------------------------------------------- 1. goldens, full mode
@pytest.fixture(scope="module")
def faulted(golden):
    """full_faults_n10_t4 with dealer 2's A_20 replaced: five round-1 complaints (verdicts 0, 0, 0, 2, 1; dealers
    3, 6, 9 leave), nine honest round-4 complaints against dealer 2."""
    cer = faulted_ceremony(golden)
    cer["s"], cer["s_prime"] = cer.pop("shares")
    return cer


def full_scenarios(cer):
    n = cer["n"]
    s, sp, c2, valid = cer["s"], cer["s_prime"], cer["c2"], cer["c4"]
    q, i, sh, rn = valid[0]
    forged = [(q, i, bump(sh), rn), (4, 5) + pair(s, sp, n, 4, 3)]  # FalseClaimedEquality, FalseClaimedInequality
    rng = random.Random(5)
    mixed4 = valid + forged + valid[3:6]
    rng.shuffle(mixed4)
    mixed2 = c2 + c2[1:3]
    rng.shuffle(mixed2)
    f3 = bytes([int(k != 4) for k in range(n)])
    return {
        "honest": (c2, valid, None),
        "none": ([], [], None),
        "forged_only": (c2[3:], forged, None),
        "one_valid_among_forged": (c2, forged + [valid[8]], None),
        "against_disqualified": (c2, valid + [(4, 3) + pair(s, sp, n, 2, 3), (1, 9, sc(5), sc(6))], None),
        "duplicates_interleaved": (mixed2, mixed4, None),
        "no_phase3_complained": (c2, valid + [(7, 5, sc(12345), sc(67890))], f3),
        "no_phase3_silent": (c2, valid, f3),
        "round4_silent": (c2, [], None),
    }


SCENARIOS = ["honest", "none", "forged_only", "one_valid_among_forged", "against_disqualified",
             "duplicates_interleaved", "no_phase3_complained", "no_phase3_silent", "round4_silent"]


@pytest.mark.parametrize("ws", [2, 3])
@pytest.mark.parametrize("name", SCENARIOS)
def test_full_goldens(be, ranks, faulted, name, ws):
    """full_faults_n10_t4 over two and three ranks under the complaint sets of
    tests/test_gpu_ceremony_proven.py: every output equals the single-context call's."""
    c2, c4, f3 = full_scenarios(faulted)[name]
    p = single_full(be, faulted, c2, c4, f3)
    sh = run_sharded(ranks, ws, faulted, c2, c4, True, None, f3)
    assert_same(sh, p, True)
    assert all(e == 3 for e in sh.evals)
    if name == "honest":
        assert p.verdict == [0, 0, 0, 2, 1] and p.verdict4 == [0] * 9 and p.result.reconstruct[1] == 1
        h = be.env_init(faulted["t"], faulted["n"], CK)
        oracle2(h, faulted, sh.verdict)
        oracle4(h, faulted, sh.verdict4)
        assert [f & 3 for f in sh.flags] == [0, FLAG_ROUND4, FLAG_ROUND2, 0, 0, FLAG_ROUND2, 0, 0, FLAG_ROUND2, 0]
    if name == "forged_only":
        assert p.verdict == [2, 1] and p.verdict4 == [3, 2]
        assert sh.fields[2] == [1] * 10 and sh.fields[5] == [0] * 10  # nobody leaves, nobody is reconstructed
    if name == "against_disqualified":
        assert sh.verdict4[-2:] == [COMPLAINT_IGNORED] * 2
    if name == "no_phase3_complained":
        assert sh.verdict4[-1] == COMPLAINT_NO_PHASE3 and sh.fields[5][4] == 1 and sh.finalise_status == FIN_OK
    if name == "no_phase3_silent":
        assert (sh.finalise_status, sh.recovery_index) == (FIN_PANIC, 4) and sh.fields[-1] == ZERO
        assert sh.flags[4] == FLAG_NO_PHASE3
    if name == "round4_silent":  # rejections alone reconstruct nobody
        assert REJECT in sh.fields[1] and sh.fields[5] == [0] * 10


@pytest.mark.parametrize("ws,name", [(2, "full_n10_t4.json"), (3, "full_n10_t4.json"), (3, "full_n4_t1.json")])
def test_full_honest_goldens(be, ranks, golden, ws, name):
    """The honest fixtures without a complaint; n = 4 over three ranks is D = 1, 1, 2."""
    cer = golden_full(golden, name)
    p = single_full(be, cer, [], [])
    sh = run_sharded(ranks, ws, cer, [], [])
    assert_same(sh, p, True)
    assert sh.fields[-1].hex() == golden(name)["mpk"] and sh.dissent == [0] * cer["n"]


# ---------------------------------------------------------------- 1b. goldens, plaintext shares
def golden_plain(golden, name):
    c = golden(name)
    return dict(n=c["n"], t=c["t"], E=H(c["E"]), A=H(c["A"]), s=H(c["s"]), s_prime=H(c["s_prime"]))


def honest4(be, cer, f1=None, f3=None):
    """One complaint per round-4 rejection of a qualified dealer, with the pair the receiver holds."""
    n = cer["n"]
    be.env_init(cer["t"], n, CK)
    ones = bytes([1] * n)
    r = be.ceremony_verify_fetched(cer["E"], cer["A"], cer["s"], cer["s_prime"], f1 or ones, f3 or ones, n, cer["t"])
    return [(j + 1, i + 1) + pair(cer["s"], cer["s_prime"], n, i, j) for i in range(n) for j in range(n)
            if r.qualified[i] and r.dec4[i * n + j] == REJECT]


@pytest.mark.parametrize("ws", [2, 3])
@pytest.mark.parametrize("name,status", [("fault_a_generator_n10_t4.json", FIN_OK),
                                         ("fault_a_many_n10_t4.json", FIN_PHASE4_ERROR),
                                         ("fault_recon_only_n10_t4.json", FIN_OK),
                                         ("fault_recon_insufficient_n16_t3.json", FIN_INSUFFICIENT),
                                         ("fault_recon_r2err_n16_t3.json", None)])
def test_plain_goldens_everyone_files(be, ranks, golden, name, status, ws):
    """The fault fixtures with every receiver's round-4 complaint: the rejection rule's outcome, which is
    the fixture's; phase4_error arises from the proven complaints, INSUFFICIENT names the first
    reconstructed dealer."""
    cer = golden_plain(golden, name)
    c4 = honest4(be, cer)
    assert c4
    p = single_plain(be, cer, c4)
    sh = run_sharded(ranks, ws, cer, [], c4, full=False)
    assert_same(sh, p, False)
    c = golden(name)
    assert sh.fields[2] == c["qualified"] and sh.fields[5] == c["reconstruct"] and sh.fields[-1].hex() == c["mpk"]
    if status is not None:
        assert sh.finalise_status == status
    if status == FIN_INSUFFICIENT:
        assert sh.recovery_index == c["reconstruct"].index(1) and sh.fields[-1] == ZERO
    if status == FIN_PHASE4_ERROR:
        silent = run_sharded(ranks, ws, cer, [], [], full=False)  # the same rows with no complaint: no such error
        assert silent.fields[7] == 0 and silent.fields[5] == [0] * cer["n"]
        assert_same(silent, single_plain(be, cer, []), False)


@pytest.mark.parametrize("ws", [2, 3])
def test_plain_where_the_rules_differ(be, ranks, golden, ws):
    """fault_a_generator (dealer 6's A row is the generator): forged complaints only, one valid among
    forged, a complaint against a dealer round 2 disqualified, absent phase-1 and phase-3 broadcasts."""
    cer = golden_plain(golden, "fault_a_generator_n10_t4.json")
    n = cer["n"]
    valid = honest4(be, cer)
    assert len(valid) == 9
    q, i, sh_, rn = valid[0]
    forged = [(q, i, sc(int.from_bytes(sh_, "little") + 1), rn), (3, 2) + pair(cer["s"], cer["s_prime"], n, 1, 2)]
    for c4, want in ((forged, [3, 2]), (forged + [valid[4]], [3, 2, 0])):
        p = single_plain(be, cer, c4)
        sh = run_sharded(ranks, ws, cer, [], c4, full=False)
        assert_same(sh, p, False)
        assert sh.verdict4 == want and sh.fields[5] == [int(k == 5 and 0 in want) for k in range(n)]
    # dealer 9's share to receiver 2 is wrong: round 2 disqualifies it, the complaint against it is ignored
    s = bytearray(cer["s"])
    k = 32 * (8 * n + 1)
    s[k:k + 32] = sc(int.from_bytes(s[k:k + 32], "little") + 1)
    bad = dict(cer, s=bytes(s))
    c4 = valid + [(4, 9) + pair(bad["s"], bad["s_prime"], n, 8, 3)]
    sh = run_sharded(ranks, ws, bad, [], c4, full=False)
    assert_same(sh, single_plain(be, bad, c4), False)
    assert sh.verdict4 == [0] * 9 + [COMPLAINT_IGNORED] and sh.fields[2] == [int(k != 8) for k in range(n)]
    # dealer 3 publishes no phase-3 broadcast, dealer 8 no phase-1 broadcast
    f1, f3 = bytes([int(k != 7) for k in range(n)]), bytes([int(k != 2) for k in range(n)])
    for c4, st in ((valid + [(7, 3, sc(1), sc(2))], (FIN_OK, -1)), (valid, (FIN_PANIC, 2))):
        p = single_plain(be, cer, c4, f1, f3)
        sh = run_sharded(ranks, ws, cer, [], c4, False, f1, f3)
        assert_same(sh, p, False)
        assert (sh.finalise_status, sh.recovery_index) == st and sh.fields[2][7] == 0
        assert sh.fields[0][7 * n:8 * n] == bytes([SELF if j == 7 else MISSING for j in range(n)])
        assert sh.flags[2] & FLAG_NO_PHASE3 and (st[0] == FIN_OK or sh.fields[-1] == ZERO)


def plain_scenarios(be, golden):
    """The plaintext cases the multi-process run repeats (tests/dist_worker_proven.py): name -> (ceremony,
    round-4 complaints, fetched1, fetched3).  golden: the fixture loader."""
    agen = golden_plain(golden, "fault_a_generator_n10_t4.json")
    n = agen["n"]
    f1, f3 = bytes([int(k != 7) for k in range(n)]), bytes([int(k != 2) for k in range(n)])
    out = {"everyone_files": (agen, honest4(be, agen), None, None),
           "no_phase3_silent": (agen, honest4(be, agen), f1, f3)}
    for key, name in (("insufficient", "fault_recon_insufficient_n16_t3.json"), ("phase4", "fault_a_many_n10_t4.json")):
        cer = golden_plain(golden, name)
        out[key] = (cer, honest4(be, cer), None, None)
    return out


FULL_DIST = ["honest", "forged_only", "duplicates_interleaved", "no_phase3_silent", "none"]
PLAIN_DIST = ["everyone_files", "no_phase3_silent", "insufficient", "phase4"]


# ---------------------------------------------------------------- 2. the swapped-share dealer
def test_swapped_share_dealer_stays(be, ranks, golden):
    """Dealer 4 sends receiver 7 its share and randomness swapped.  The receiver rejects, but its honest
    proof fails ProofOfMisbehaviour::verify's own check h*share + g*randomness (broadcast.rs:271-283):
    verdict 1, the dealer stays qualified on every rank, and dissent is 1 for that receiver."""
    c = golden("full_n10_t4.json")
    n, t = c["n"], c["t"]
    i, q = 3, 6
    be.env_init(t, n, CK)
    a, b = dkg_amd.dealer_coefficients(H(c["master_seed"]), c["ceremony"], 0, n, t)
    E, A, s, sp = be.share_gen(a, b, n, n, t)
    s, sp = bytearray(s), bytearray(sp)
    k = 32 * (i * n + q)
    s[k:k + 32], sp[k:k + 32] = sp[k:k + 32], s[k:k + 32]
    sk, pk = H(c["member_sk"]), H(c["member_pk"])
    e1, ct = be.encrypt_shares(pk, bytes(s), bytes(sp), H(c["enc_r"]), n, n)
    cer = dict(n=n, t=t, E=E, A=A, e1=e1, ct=ct, sk=sk, pk=pk)
    proof = be.complaints_prove(sk[32 * q:32 * q + 32], enc_of(e1, ct, n, i, q), bytes(range(64)))
    c2 = [(q + 1, i + 1, proof)]
    p = single_full(be, cer, c2, [])
    assert p.verdict == [1] and p.result.dec2[i * n + q] == REJECT and p.result.qualified == [1] * n
    assert p.dissent == [int(j == q) for j in range(n)]
    for ws in (2, 3):
        sh = run_sharded(ranks, ws, cer, c2, [])
        assert_same(sh, p, True)
        assert sh.flags == [0] * n


# ---------------------------------------------------------------- 3. the index into the pass's R
DEALERS = [1, 43, 44, 63, 64, 65, 66, 86, 87, 130]  # first / last of each rank at ws = 2 and 3; the 64-column boundary
ACCUSERS = [1, 64, 65, 130]
R2BAD, R4BAD = (43, 64, 87), (1, 44, 65, 130)


@pytest.fixture(scope="module")
def c130(be):
    """n = 130, t = 64 from seeds, as the c130 fixture of tests/test_gpu_shard_full.py: 65 dealers per rank
    at ws = 2 (a shard crosses the 64-dealer column group), 43 / 43 / 44 at ws = 3.  The share ciphertexts
    dealers 43, 64, 87 sent the four accusers are flipped (valid round-1 complaints), A_i0 of dealers 1, 44,
    65, 130 is replaced (valid round-4 complaints); every other complaint is false."""
    from tests.test_gpu_shard_full import Committee

    c = Committee(be, 130, 64, 0x41)
    n, t, N = c.n, c.t, c.t + 1
    ct, A = bytearray(c.ct), bytearray(c.A)
    for i in R2BAD:
        for j in ACCUSERS:
            ct[32 * (2 * ((i - 1) * n + j - 1) + 1) + 7] ^= 0x20
    for i in R4BAD:
        A[32 * N * (i - 1):32 * N * (i - 1) + 32] = O.base_mul(sc(900 + i))
    cer = dict(n=n, t=t, E=c.E, A=bytes(A), e1=c.e1, ct=bytes(ct), sk=c.sk, pk=c.pk)
    ref = be.ceremony_verify_full(cer["E"], cer["A"], cer["e1"], cer["ct"], cer["sk"], n, t)
    pairs = [(j, i) for i in DEALERS for j in ACCUSERS if i != j]
    rng = random.Random(130)
    proofs = be.complaints_prove(b"".join(c.sk[32 * (j - 1):32 * j] for j, _ in pairs),
                                 b"".join(enc_of(cer["e1"], cer["ct"], n, i - 1, j - 1) for j, i in pairs),
                                 bytes(rng.randrange(256) for _ in range(64 * len(pairs))))
    c2 = [(j, i, proofs[192 * k:192 * k + 192]) for k, (j, i) in enumerate(pairs)]
    c4 = [(j, i) + pair(ref.s, ref.s_prime, n, i - 1, j - 1) for j, i in pairs]
    p = single_full(be, cer, c2, c4)
    assert p.verdict == [0 if i in R2BAD else 2 for _, i in pairs]
    assert p.verdict4 == [COMPLAINT_IGNORED if i in R2BAD else 0 if i in R4BAD else 2 for _, i in pairs]
    assert p.finalise_status == FIN_OK and sum(p.result.reconstruct) == 4 and p.result.n_qualified == n - 3
    return cer, c2, c4, p


@pytest.mark.parametrize("ws", [2, 3])
@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("split", [1, 2, 4])
def test_index_mapping(ranks, c130, split, streams, ws):
    """The complaints read the rank's own pass (source 3) unsplit, and with 2 and 4 pieces, where the pass
    holds b_j P(j) and `scale` is in play; one chunk stream and two."""
    cer, c2, c4, p = c130
    try:
        for b in ranks:
            b.set_split(split)
            b.set_streams(streams)
        sh = run_sharded(ranks, ws, cer, c2, c4)
        assert sh.evals == [3] * ws
        assert [ranks[r].last_split() for r in range(ws)] == [split] * ws
    finally:
        for b in ranks:
            b.set_split(0)
            b.set_streams(2)
    assert_same(sh, p, True)


@pytest.mark.parametrize("mode", [1, 2])
def test_index_mapping_against_forced_sources(ranks, c130, mode):
    """Horner walks (1) and second tables (2) forced in the new calls give the same verdicts as source 3."""
    cer, c2, c4, p = c130
    try:
        for b in ranks:
            b.set_complaint_eval(mode)
        sh = run_sharded(ranks, 3, cer, c2, c4)
    finally:
        for b in ranks:
            b.set_complaint_eval(0)
    assert sh.evals == [mode] * 3
    assert_same(sh, p, True)


# ---------------------------------------------------------------- 4. fallbacks
@pytest.mark.parametrize("knob", ["overlap", "interpolation"])
def test_fallbacks(be, ranks, faulted, knob):
    """Protocol-order rounds and interpolation hold no R with both rounds' evaluations: the call falls back
    to the Horner / tables switch, with the same outputs."""
    c2, c4, _ = full_scenarios(faulted)["duplicates_interleaved"]
    p = single_full(be, faulted, c2, c4)
    try:
        for b in ranks:
            b.set_overlap(False) if knob == "overlap" else b.set_verify_mode(1)
        sh = run_sharded(ranks, 2, faulted, c2, c4)
    finally:
        for b in ranks:
            b.set_overlap(True)
            b.set_verify_mode(0)
    assert all(e in (1, 2, 12) for e in sh.evals)
    assert_same(sh, p, True)


# ---------------------------------------------------------------- 5. the binomial's rerun
def test_binomial_rerun_reruns_the_complaints(be, ranks, golden):
    """n = 64 (the shape of test_binomial_dedicated_redo): an all-identity E / A row in rank 0, which also owns
    round-4 complaints.  The dedicated per-step binomial marks its word, the rank reruns its verification
    with the complete formula and the complaint stage with it: verdicts and outcome equal the
    complete-formula run's and the single context's."""
    cer = golden_plain(golden, "ceremony_n64_t31.json")
    n, N = cer["n"], cer["t"] + 1
    E, A = bytearray(cer["E"]), bytearray(cer["A"])
    for buf in (E, A):
        buf[32 * N * 5:32 * N * 6] = bytes(32 * N)
    A[32 * N * 7:32 * N * 7 + 32] = O.base_mul(sc(77))  # dealer 8: a valid complaint; dealer 40 (rank 1) as well
    A[32 * N * 39:32 * N * 39 + 32] = O.base_mul(sc(78))
    cer = dict(cer, E=bytes(E), A=bytes(A))
    c4 = [(j, i) + pair(cer["s"], cer["s_prime"], n, i - 1, j - 1) for j, i in ((2, 8), (9, 6), (3, 4), (1, 40), (64, 33))]
    p = single_plain(be, cer, c4)
    assert p.verdict4 == [0, COMPLAINT_IGNORED, 2, 0, 2]
    outs = {}
    try:
        for formula in (0, 1):
            for b in ranks:
                b.set_split(1)
                b.set_binomial(1)
                b.set_stepping_formula(formula)
            outs[formula] = run_sharded(ranks, 2, cer, [], c4, full=False)
    finally:
        for b in ranks:
            b.set_split(0)
            b.set_binomial(0)
            b.set_stepping_formula(0)
    assert outs[0].reruns == [1, 0] and outs[1].reruns == [0, 0]
    assert outs[0].evals == [3, 3]
    for sh in outs.values():
        assert_same(sh, p, False)
    assert (outs[0].fields, outs[0].per_rank, outs[0].flags) == (outs[1].fields, outs[1].per_rank, outs[1].flags)


# ---------------------------------------------------------------- 6. interface edges
def u32s(xs):
    return (ctypes.c_uint32 * max(len(xs), 1))(*xs)


def raw_full(b, cer, d0, d1, C, acc, acd, proofs, C4, acc4, acd4, sh4, rn4, verdict, verdict4, flag_rows=None,
             pk=True):
    """dkg_ceremony_shard_verify_full_proven_device through the C ABI: (rc, flags, dissent, dec2)."""
    import torch

    n, t = cer["n"], cer["t"]
    N, D = t + 1, d1 - d0
    R = D if flag_rows is None else flag_rows
    u8 = dict(dtype=torch.uint8, device="cuda:0")
    ins = [_dev(cer[k][w * d0:w * d1]) for k, w in (("E", 32 * N), ("A", 32 * N), ("e1", 64 * n), ("ct", 64 * n))]
    o2, o4, oA, op = (torch.zeros(max(D * n, 32 * n), **u8) for _ in range(4))
    fl = torch.full((max(R, 1),), -1, dtype=torch.int32, device="cuda:0")
    ds = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    vp = ctypes.c_void_p
    rc = _lib.lib().dkg_ceremony_shard_verify_full_proven_device(
        b.ctx, n, t, d0, d1, *(vp(x.data_ptr()) for x in ins), cer["sk"], cer["pk"] if pk else None, None, None, C, acc,
        acd, proofs, C4, acc4, acd4, sh4, rn4, vp(o2.data_ptr()), vp(o4.data_ptr()), vp(oA.data_ptr()), vp(op.data_ptr()),
        R, vp(fl.data_ptr()), vp(ds.data_ptr()), verdict, verdict4, None)
    return rc, fl.tolist()[:R], ds.tolist(), _host(o2)[:D * n], _host(op)[:32 * n]


def test_no_complaints_null_arrays_and_empty_rank(ranks, faulted):
    """C == 0 / C4 == 0 with null arrays applies the proven rule (nobody leaves but MISSING rows, nobody is
    reconstructed); a rank without dealers (d0 == d1) writes zero flags, zero dissent and a zero partial."""
    b = ranks[0]
    cer = faulted
    n = cer["n"]
    b.env_init(cer["t"], n, CK)
    rc, fl, ds, d2, _ = raw_full(b, cer, 0, 5, 0, None, None, None, 0, None, None, None, None, None, None)
    assert rc == DKG_OK and fl == [0] * 5 and b.last_complaint_eval() == 3
    want = [sum(d2[i * n + j] == REJECT for i in range(5)) for j in range(n)]
    assert ds == want and sum(want) == 1  # dealer 3 -> receiver 5, the one round-2 rejection among dealers 1..5
    v2, v4 = (ctypes.c_int32 * 5)(*[9] * 5), (ctypes.c_int32 * 9)(*[9] * 9)
    a2, d2_, pr = lists2(cer["c2"])
    a4, d4_, s4, r4 = lists4(cer["c4"])
    rc, fl, ds, _, part = raw_full(b, cer, 4, 4, 5, u32s(a2), u32s(d2_), pr, 9, u32s(a4), u32s(d4_), s4, r4, v2, v4, 4)
    assert rc == DKG_OK and fl == [0] * 4 and ds == [0] * n and part == bytes(32 * n)
    assert list(v2) == [COMPLAINT_NOT_OWNED] * 5 and list(v4) == [COMPLAINT_NOT_OWNED] * 9


def test_bad_arguments(ranks, faulted):
    b = ranks[0]
    cer = faulted
    n = cer["n"]
    b.env_init(cer["t"], n, CK)
    a2, d2, pr = lists2(cer["c2"])
    a4, d4, s4, r4 = lists4(cer["c4"])
    v2, v4 = (ctypes.c_int32 * 5)(), (ctypes.c_int32 * 9)()
    good = dict(C=5, acc=u32s(a2), acd=u32s(d2), proofs=pr, C4=9, acc4=u32s(a4), acd4=u32s(d4), sh4=s4, rn4=r4,
                verdict=v2, verdict4=v4)
    bad = [dict(acd=u32s([0] + d2[1:])), dict(acc=u32s(a2[:4] + [n + 1])), dict(acd4=u32s(d4[:8] + [n + 1])),
           dict(acc4=u32s([0] + a4[1:])), dict(proofs=None), dict(verdict=None), dict(sh4=None), dict(rn4=None),
           dict(verdict4=None), dict(acc=None), dict(acd4=None), dict(flag_rows=4), dict(pk=False)]
    for over in bad:
        rc = raw_full(b, cer, 0, 5, **dict(good, **over))[0]
        assert rc == DKG_E_ARG, over
    assert raw_full(b, cer, 0, 5, **good)[0] == DKG_OK  # and the context still serves the next call
    assert list(v2) == [COMPLAINT_NOT_OWNED, COMPLAINT_NOT_OWNED, 0, 2, 1]  # accused 9, 6, 3, 2, 2; dealers 1..5 here
    with pytest.raises(dkg_amd.DkgError):
        b.set_complaint_eval(3)  # source 3 cannot be forced


def test_existing_shard_calls_unchanged_around_a_proven_call(ranks, faulted):
    """The rejection-rule shard call on the same context before and after a proven call: the same rows,
    terms and partial sums."""
    import torch

    b = ranks[0]
    cer = faulted
    n, t = cer["n"], cer["t"]
    N = t + 1
    b.env_init(t, n, CK)

    def old():
        u8 = dict(dtype=torch.uint8, device="cuda:0")
        ins = [_dev(cer[k][w * 0:w * 5]) for k, w in (("E", 32 * N), ("A", 32 * N), ("e1", 64 * n), ("ct", 64 * n))]
        outs = [torch.zeros(5 * n, **u8), torch.zeros(5 * n, **u8), torch.zeros(5 * 32, **u8), torch.zeros(n * 32, **u8)]
        b.ceremony_shard_verify_full_device(n, t, 0, 5, *(x.data_ptr() for x in ins), cer["sk"],
                                            *(x.data_ptr() for x in outs))
        return [_host(x) for x in outs]

    before = old()
    sh = run_sharded(ranks, 2, cer, cer["c2"], cer["c4"])
    assert sh.evals == [3, 3]
    assert old() == before
    # the rejection rule drops dealer 3 from the partial sums on the strength of receiver 5's REJECT alone
    assert before[0][2 * n + 4] == REJECT


# ---------------------------------------------------------------- 6b. the in-library multi-device driver
@pytest.fixture(scope="module", params=[[0, 0], [0, 0, 0]], ids=lambda d: f"ws{len(d)}")
def mb(request):
    m = dkg_amd.MultiBackend(request.param)
    yield m
    m.close()


def same_proven(got, want, full):
    assert _fields(got.result) == _fields(want.result)
    assert (got.verdict4, got.finalise_status, got.recovery_index) == (want.verdict4, want.finalise_status,
                                                                       want.recovery_index)
    if full:
        assert (got.verdict, got.dissent) == (want.verdict, want.dissent)


@pytest.mark.parametrize("name", ["honest", "forged_only", "duplicates_interleaved", "no_phase3_silent", "none"])
def test_multi_backend_full(be, mb, faulted, name):
    """dkg_multi_ceremony_verify_full_proven: every output equals the single-context call's."""
    cer = faulted
    c2, c4, f3 = full_scenarios(cer)[name]
    want = single_full(be, cer, c2, c4, f3)
    mb.env_init(cer["t"], cer["n"], CK)
    got = mb.ceremony_verify_full_proven(cer["E"], cer["A"], cer["e1"], cer["ct"], cer["sk"], cer["pk"], *lists2(c2),
                                         *lists4(c4), cer["n"], cer["t"], fetched3=f3)
    same_proven(got, want, True)
    assert [mb.shard(i).last_complaint_eval() for i in range(len(mb))] == [3] * len(mb)


@pytest.mark.parametrize("name", ["fault_a_generator_n10_t4.json", "fault_recon_insufficient_n16_t3.json",
                                  "fault_a_many_n10_t4.json"])
def test_multi_backend_plain(be, mb, golden, name):
    """dkg_multi_ceremony_verify_proven on the fault fixtures with every receiver's complaint, and with a
    dealer that publishes no phase-3 broadcast and is complained about by nobody (PANIC, no mpk)."""
    cer = golden_plain(golden, name)
    n, t = cer["n"], cer["t"]
    c4 = honest4(be, cer)
    f3 = bytes([int(k != 6) for k in range(n)])
    mb.env_init(t, n, CK)
    for m1, m3 in ((None, None), (None, f3)):
        want = single_plain(be, cer, c4, m1, m3)
        got = mb.ceremony_verify_proven(cer["E"], cer["A"], cer["s"], cer["s_prime"], m1, m3, *lists4(c4), n, t)
        same_proven(got, want, False)
    if name == "fault_a_generator_n10_t4.json":
        assert (got.finalise_status, got.recovery_index, got.result.mpk) == (FIN_PANIC, 6, ZERO)
    lib = _lib.lib()
    o, _bufs = mb._out(n, t)
    a4, d4, s4, r4 = lists4(c4)
    rc = lib.dkg_multi_ceremony_verify_proven(mb._m, n, t, cer["E"], cer["A"], cer["s"], cer["s_prime"], None, None,
                                              len(c4), u32s(a4), u32s(d4), s4, r4, ctypes.byref(o), None, None, None)
    assert rc == DKG_E_ARG  # complaints without a verdict array


# ---------------------------------------------------------------- 6c. the six shard entry points, one driver
OUTS = ["dec2", "dec4", "A0", "partial"]
# kind -> (entry point, its arguments after d1 in order, the device pointers it requires of a rank with
# dealers).  d_partial, the host keys it takes and d_flags (flag_rows > 0) are required of every rank.
SIX = {
    "gen": ("dkg_ceremony_shard_device", ["a", "b"] + OUTS, ["a", "b"]),
    "verify": ("dkg_ceremony_shard_verify_device", ["E", "A", "s", "sp"] + OUTS, ["E", "A", "s", "sp"]),
    "gen_full": ("dkg_ceremony_shard_full_device", ["a", "b", "r", "sk", "pk", "e1_out", "ct_out"] + OUTS,
                 ["a", "b", "r"]),
    "verify_full": ("dkg_ceremony_shard_verify_full_device", ["E", "A", "e1", "ct", "sk"] + OUTS,
                    ["E", "A", "e1", "ct"]),
    "verify_proven": ("dkg_ceremony_shard_verify_proven_device",
                      ["E", "A", "s", "sp", "f1", "f3", "C4", "acc4", "acd4", "sh4", "rn4"] + OUTS +
                      ["flag_rows", "flags", "v4"], ["E", "A", "s", "sp"]),
    "verify_full_proven": ("dkg_ceremony_shard_verify_full_proven_device",
                           ["E", "A", "e1", "ct", "sk", "pk", "f1", "f3", "C", "acc", "acd", "proofs", "C4", "acc4",
                            "acd4", "sh4", "rn4"] + OUTS + ["flag_rows", "flags", "dissent", "v2", "v4"],
                           ["E", "A", "e1", "ct"]),
}
ALWAYS = ["partial", "sk", "pk", "flags"]


def six_call(b, kind, cer, seeds, d0, d1, R, null=None):
    """One of the six entry points through the C ABI on dealers [d0, d1) of the faulted ceremony `cer` (the
    received broadcasts and complaint lists) or of `seeds` (full_n10_t4.json: the generate modes), with
    argument `null` passed as NULL.  Every output buffer is poisoned first.  -> (rc, {output: bytes / list})."""
    import torch

    n, t = cer["n"], cer["t"]
    N, D = t + 1, d1 - d0
    fn, order, _ = SIX[kind]
    u8 = dict(dtype=torch.uint8, device="cuda:0")
    gen = kind.startswith("gen")
    a, b_ = dkg_amd.dealer_coefficients(H(seeds["master_seed"]), seeds["ceremony"], d0, D, t) if D else (b"", b"")
    host = dict(a=a, b=b_, r=H(seeds["enc_r"])[64 * n * d0:64 * n * d1], E=cer["E"][32 * N * d0:32 * N * d1],
                A=cer["A"][32 * N * d0:32 * N * d1], s=cer["s"][32 * n * d0:32 * n * d1],
                sp=cer["s_prime"][32 * n * d0:32 * n * d1], e1=cer["e1"][64 * n * d0:64 * n * d1],
                ct=cer["ct"][64 * n * d0:64 * n * d1])
    ins = {k: _dev(v) for k, v in host.items() if k in order}
    size = dict(dec2=D * n, dec4=D * n, A0=32 * D, partial=32 * n, e1_out=64 * D * n, ct_out=64 * D * n,
                flags=4 * R, dissent=4 * n)
    outs = {k: torch.full((max(v, 16),), 0xEE, **u8) for k, v in size.items() if k in order}
    a2, d2, pr = lists2(cer["c2"])
    a4, d4, s4, r4 = lists4(cer["c4"])
    v2, v4 = (ctypes.c_int32 * len(a2))(*[9] * len(a2)), (ctypes.c_int32 * len(a4))(*[9] * len(a4))
    args = {k: ctypes.c_void_p(v.data_ptr()) for k, v in (ins | outs).items()}
    args.update(sk=H(seeds["member_sk"]) if gen else cer["sk"], pk=H(seeds["member_pk"]) if gen else cer["pk"], f1=None,
                f3=None, C=len(a2), acc=u32s(a2), acd=u32s(d2), proofs=pr, C4=len(a4), acc4=u32s(a4), acd4=u32s(d4),
                sh4=s4, rn4=r4, flag_rows=R, v2=v2, v4=v4)
    if null is not None:
        assert null in order
        args[null] = None
    rc = getattr(_lib.lib(), fn)(b.ctx, n, t, d0, d1, *(args[k] for k in order), None)
    got = {k: _host(v)[:size[k]] for k, v in outs.items()}
    if "v4" in order:
        got["v4"] = list(v4)
    if "v2" in order:
        got["v2"] = list(v2)
    return rc, got


@pytest.fixture(scope="module")
def six_fresh(faulted, golden):
    """(kind, d0, d1, R) -> the call's outputs on a context of its own, computed once."""
    seeds = golden("full_n10_t4.json")
    memo = {}

    def get(kind, d0, d1, R):
        key = (kind, d0, d1, R)
        if key not in memo:
            b = dkg_amd.Backend(0)
            try:
                b.env_init(faulted["t"], faulted["n"], CK)
                rc, memo[key] = six_call(b, kind, faulted, seeds, d0, d1, R)
                assert rc == DKG_OK, key
            finally:
                b.close()
        return memo[key]

    return get


def six_sequence():
    """(kind, ws, rank): a 3-dealer rank, then all 10 dealers (the merged buffers grow), the 3-dealer rank
    again (they are reused), the last ranks of two and of three (5 and 4 dealers), and a rank without dealers."""
    kinds = list(SIX)
    seq = [(k, 3, 1) for k in kinds] + [(k, 1, 0) for k in kinds] + [(k, 3, 0) for k in kinds]
    seq += [(k, 2, 1) for k in kinds[::2]] + [(k, 3, 2) for k in kinds[1::2]] + [(k, 3, None) for k in kinds]
    return seq


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_six_entry_points_share_one_context(faulted, golden, six_fresh, order):
    """The six entry points one after another on ONE context, in one order and in the reverse one: every
    output (rows, terms, partial sums, flags, dissent, verdicts, ciphertexts) is what the same call gives
    on a fresh context, whatever the calls before it left in the context's buffers."""
    n, t = faulted["n"], faulted["t"]
    assert [shard_range(n, 3, r) for r in range(3)] == [(0, 3), (3, 6), (6, 10)]
    seeds = golden("full_n10_t4.json")
    seq = six_sequence()
    b = dkg_amd.Backend(0)
    try:
        b.env_init(t, n, CK)
        for kind, ws, r in seq if order == "forward" else seq[::-1]:
            d0, d1 = (4, 4) if r is None else shard_range(n, ws, r)
            R = shard_rows(n, ws)
            rc, got = six_call(b, kind, faulted, seeds, d0, d1, R)
            assert rc == DKG_OK, (kind, ws, r)
            assert got == six_fresh(kind, d0, d1, R), (kind, ws, r)
            if r is None:
                assert got["partial"] == bytes(32 * n)
    finally:
        b.close()
    # the generated ciphertexts are the fixture's rows, the received ones' verdicts the single context's
    g = six_fresh("gen_full", 3, 6, 4)
    assert (g["e1_out"].hex(), g["ct_out"].hex()) == (seeds["e1"][128 * n * 3:128 * n * 6],
                                                      seeds["ct"][128 * n * 3:128 * n * 6])
    assert six_fresh("verify_full_proven", 0, 10, 10)["v2"] == [0, 0, 0, 2, 1]


@pytest.mark.parametrize("kind", list(SIX))
def test_six_entry_points_required_pointers(faulted, golden, six_fresh, kind):
    """One argument rule for the six: with dealers, each required pointer NULL in turn is DKG_E_ARG and the
    context then serves the good call with unchanged outputs; a rank without dealers (d0 == d1) takes the
    same NULLs, except d_partial (written even then), the host keys and d_flags."""
    n, t = faulted["n"], faulted["t"]
    seeds = golden("full_n10_t4.json")
    _, order, inputs = SIX[kind]
    always = [k for k in ALWAYS if k in order]
    b = dkg_amd.Backend(0)
    try:
        b.env_init(t, n, CK)
        for null in inputs + ["dec2", "dec4", "A0"] + always:
            assert six_call(b, kind, faulted, seeds, 6, 10, 4, null)[0] == DKG_E_ARG, null
        rc, got = six_call(b, kind, faulted, seeds, 6, 10, 4)
        assert rc == DKG_OK and got == six_fresh(kind, 6, 10, 4)
        empty = six_fresh(kind, 4, 4, 4)
        for null in inputs + ["dec2", "dec4", "A0"]:
            rc, got = six_call(b, kind, faulted, seeds, 4, 4, 4, null)
            assert rc == DKG_OK and got == empty, null
        for null in always:
            assert six_call(b, kind, faulted, seeds, 4, 4, 4, null)[0] == DKG_E_ARG, null
        assert six_call(b, kind, faulted, seeds, 6, 10, 4)[1] == six_fresh(kind, 6, 10, 4)
    finally:
        b.close()


# ---------------------------------------------------------------- 7. the headline shape, once
def test_rank0_of_8_at_n1024_matches_single_context(be, ranks):
    """n = 1024, t = 511, rank 0 of 8 (128 dealers, two column groups), one complaint of each round per
    dealer: verdicts, flags and the dissent partial against the single-context call on the same ceremony."""
    import torch

    n, t = 1024, 511
    N, D = t + 1, 128
    master = bytes(range(32))
    be.env_init(t, n, CK)
    u8 = dict(dtype=torch.uint8, device="cuda:0")
    ta, tb = torch.empty(32 * n * N, **u8), torch.empty(32 * n * N, **u8)
    tr = torch.empty(64 * n * n, **u8)
    be.dealer_coefficients_device(master, 7, 1, 0, n, t, ta.data_ptr(), tb.data_ptr())
    be.enc_randomness_device(master, 7, 1, 0, n, n, t, tr.data_ptr())
    sk, pk = be.member_keys(master, 7, n)
    E, A, s, sp = be.share_gen(_host(ta), _host(tb), n, n, t)
    e1, ct = be.encrypt_shares(pk, s, sp, _host(tr), n, n)
    ct, A = bytearray(ct), bytearray(A)
    pairs = [((37 * i + 5) % n + 1, i + 1) for i in range(D)]  # (accuser, accused), never the dealer itself
    assert all(j != i for j, i in pairs)
    r2bad, r4bad = {3, 64, 65, 128}, {1, 63, 66, 127}
    for j, i in pairs:
        if i in r2bad:
            ct[32 * (2 * ((i - 1) * n + j - 1) + 1) + 3] ^= 1
        if i in r4bad:
            A[32 * N * (i - 1):32 * N * (i - 1) + 32] = O.base_mul(sc(4000 + i))
    ct, A = bytes(ct), bytes(A)
    proofs = be.complaints_prove(b"".join(sk[32 * (j - 1):32 * j] for j, _ in pairs),
                                 b"".join(enc_of(e1, ct, n, i - 1, j - 1) for j, i in pairs), bytes([7]) * (64 * D))
    c2 = [(j, i, proofs[192 * k:192 * k + 192]) for k, (j, i) in enumerate(pairs)]
    # the round-4 complaints disclose what the accuser decrypts: the plaintext pair, the share flipped where
    # the ciphertext was
    c4 = []
    for j, i in pairs:
        sh_, rn = pair(s, sp, n, i - 1, j - 1)
        if i in r2bad:
            v = bytearray(sh_)
            v[3] ^= 1
            sh_ = bytes(v)
        c4.append((j, i, sh_, rn))
    p = be.ceremony_verify_full_proven(E, A, e1, ct, sk, pk, *lists2(c2), *lists4(c4), n, t)
    assert p.verdict == [0 if i in r2bad else 2 for _, i in pairs]
    assert p.verdict4 == [COMPLAINT_IGNORED if i in r2bad else 0 if i in r4bad else 2 for _, i in pairs]
    b = ranks[0]
    b.env_init(t, n, CK)
    ins = [_dev(x[w * 0:w * D]) for x, w in ((E, 32 * N), (A, 32 * N), (e1, 64 * n), (ct, 64 * n))]
    o2, o4 = torch.zeros(D * n, **u8), torch.zeros(D * n, **u8)
    oA, op = torch.zeros(D * 32, **u8), torch.zeros(n * 32, **u8)
    fl = torch.full((D,), -1, dtype=torch.int32, device="cuda:0")
    ds = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    _, v2, v4 = b.ceremony_shard_verify_full_proven_device(
        n, t, 0, D, *(x.data_ptr() for x in ins), sk, pk, *lists2(c2), *lists4(c4), o2.data_ptr(), o4.data_ptr(),
        oA.data_ptr(), op.data_ptr(), D, fl.data_ptr(), ds.data_ptr())
    assert b.last_complaint_eval() == 3
    assert (v2, v4) == (p.verdict, p.verdict4)
    assert fl.tolist() == [(FLAG_ROUND2 if i in r2bad else 0) | (FLAG_ROUND4 if i in r4bad else 0)
                           for i in range(1, D + 1)]
    assert _host(o2) == bytes(p.result.dec2[:D * n])
    # every rejection among these dealers has its proven complaint: no dissent in this rank's partial
    assert ds.tolist() == [0] * n and p.dissent == [0] * n
    assert p.result.qualified[:D] == [int(i not in r2bad) for i in range(1, D + 1)]
