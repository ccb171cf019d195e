"""Hosted seats through rounds 3-5: dkg_complaints_verify_ceremonies, dkg_complaints3_verify_ceremonies,
dkg_party_round3_seats and dkg_finalise_seats (k_seat_lagrange) against the fixtures, tests/finalise_ref.py,
the per-ceremony calls and ceremony_batch_verify_full_proven, bit for bit."""
import random

import pytest

import dkg_amd
from dkg_amd import COMPLAINT_IGNORED, COMPLAINT_NO_PHASE3, DkgError
from tests import finalise_ref as FR
from tests import oracle_lib as O
from tests.test_gpu import CK, H, L
from tests.test_gpu_batch_proven import faulted_ceremony, full_args, golden_full
from tests.test_gpu_complaints import enc_of
from tests.test_gpu_seats import Stack, both, seat_cols, stack10  # noqa: F401 (stack10 is a fixture)

pytestmark = pytest.mark.gpu

NAMES = {"OK": 0, "R2_ERROR": 1, "R4_ERROR": 2, "PHASE4_ERROR": 3, "INSUFFICIENT": 4, "PANIC": 5}
BAD = b"\xff" * 32  # not a point


@pytest.fixture(scope="module")
def be():
    b = dkg_amd.Backend(0)
    yield b
    b.set_complaint_eval(0)
    b.close()


def ints(xs):
    return [int(bool(x)) for x in xs]


class Cer:
    """One ceremony's finalise inputs: sets, A_i0 and the share matrix s [n][n][32]."""

    def __init__(self, n, t, qualified, recon, A, s, r2=None, r4=None):
        self.n, self.t, self.q, self.r, self.s = n, t, ints(qualified), ints(recon), s
        self.A0 = [A[32 * (t + 1) * i:32 * (t + 1) * i + 32] for i in range(n)]
        self.r2, self.r4 = ints(r2 or [0] * n), ints(r4 or [0] * n)

    @classmethod
    def of(cls, c, recon=None):
        return cls(c["n"], c["t"], c["qualified"], c["reconstruct"] if recon is None else recon, H(c["A"]), H(c["s"]),
                   c["r2_error"], c["r4_error"])

    def share_bytes(self, i, j):
        return self.s[32 * (i * self.n + j):32 * (i * self.n + j) + 32]

    def share(self, i, j):
        return int.from_bytes(self.share_bytes(i, j), "little")

    def final(self, q):
        return self.q[q] and not self.r[q]

    def senders(self, disclosed=None, r2=None, r4=None):
        """The parties whose phase-5 broadcast exists and was fetched (committee.rs:684, 763-775)."""
        r2, r4 = r2 or self.r2, r4 or self.r4
        return [q for q in range(self.n) if self.final(q) and not r2[q] and not r4[q] and (disclosed is None or disclosed[q])]

    def entries(self, g, senders, keep=lambda q, i: True):
        return [(g, q + 1, i + 1, self.share_bytes(i, q)) for i in range(self.n) if self.r[i] for q in senders if keep(q, i)]


def expect_seat(c, p, disclosed=None, r2=None, r4=None):
    st, idx, mpk = FR.party_finalise(p, c.n, c.t, c.q, c.r, c.A0, c.share, disclosed=disclosed, r2_error=r2 or c.r2,
                                     r4_error=r4 or c.r4)
    return NAMES[st], idx, mpk or bytes(32)


def run_seats(be, cers, seats, entries, r2=None, r4=None, A0=None, fetched3=None, sets=None):
    """finalise_seats over stacked ceremonies `cers` (Cer objects) as [(status, index, mpk)] per seat."""
    n, t = cers[0].n, cers[0].t
    q, r = sets or (bytes(x for c in cers for x in c.q), bytes(x for c in cers for x in c.r))
    A0 = A0 or b"".join(a for c in cers for a in c.A0)
    pf = be.finalise_seats(len(cers), n, t, [g for g, _ in seats], [j for _, j in seats], q, r, A0,
                           seat_cols([c.s for c in cers], n, seats), entries, fetched3=fetched3,
                           r2_error=r2 if r2 is not None else [cers[g].r2[j] for g, j in seats],
                           r4_error=r4 if r4 is not None else [cers[g].r4[j] for g, j in seats])
    return list(zip(pf.status, pf.recovery_index, pf.mpk))


# ---------------------------------------------------------------- 1. the golden stack, all 100 seats shuffled
def test_golden_stack(be, stack10):
    st = stack10
    n, t, B = st.n, st.t, st.B
    seats = [(g, j) for g in range(B) for j in range(n)]
    random.Random(5).shuffle(seats)
    cer, js = [g for g, _ in seats], [j for _, j in seats]
    fs, ps = both(be, lambda: be.party_round3_seats(B, n, t, cer, js, st.qual, seat_cols(st.s, n, seats)))
    assert fs == b"".join(H(st.f[g]["final_share"])[32 * j:32 * j + 32] for g, j in seats)
    assert ps == b"".join(H(st.f[g]["public_share"])[32 * j:32 * j + 32] for g, j in seats)
    assert be.party_round3_seats(B, n, t, cer, js, st.qual, seat_cols(st.s, n, seats), public=False) == (fs, None)
    cers = [Cer.of(c) for c in st.f]
    entries = [e for g, c in enumerate(cers) for e in c.entries(g, c.senders())]
    assert entries
    random.Random(6).shuffle(entries)
    got = both(be, lambda: run_seats(be, cers, seats, entries))
    statuses = set()
    for (g, j), res in zip(seats, got):
        assert res == expect_seat(cers[g], j), (g, j)
        statuses.add(res[0])
        if res[0] == NAMES["OK"] and cers[g].final(j):
            assert res[2].hex() == st.f[g]["mpk"], (g, j)
    assert {NAMES["OK"], NAMES["PHASE4_ERROR"], NAMES["PANIC"]} <= statuses
    many = [g for g, c in enumerate(st.f) if c["phase4_error"] and sum(c["reconstruct"]) > 4]
    assert many  # fault_a_many: PHASE4_ERROR for every seat whose own rounds went through
    m_seats = [(many[0], j) for j in range(n)]
    got = run_seats(be, cers, m_seats, entries, r2=[0] * n, r4=[0] * n)
    assert got == [(NAMES["PHASE4_ERROR"], -1, bytes(32))] * n


# ---------------------------------------------------------------- 2. the libsodium per-party cases
@pytest.mark.parametrize("name", ["finalise_parties_n10_t4.json", "finalise_parties_recon_n10_t4.json"])
def test_fixture_cases(be, golden, name):
    f = golden(name)
    c = Cer.of(golden(f["source"]))
    n = c.n
    seats = [(0, j) for j in range(n)]
    for case in f["cases"]:
        r2, r4 = case.get("r2_error") or [0] * n, case.get("r4_error") or [0] * n
        entries = c.entries(0, c.senders(case.get("disclosed"), r2, r4))
        got = run_seats(be, [c], seats, entries, r2=r2, r4=r4)
        assert [x[0] for x in got] == [NAMES[x] for x in case["status"]], case["name"]
        assert [x[1] for x in got] == case["index"], case["name"]
        assert [x[2].hex() for x in got] == case["mpk"], case["name"]


# ---------------------------------------------------------------- 3. disclosures per (sender, dealer)
def finalise_by_pairs(c, p, keep):
    """party_finalise's loop with a per-(sender, dealer) predicate on what was fetched."""
    if sum(c.q) - sum(c.r) <= c.t:
        return NAMES["PHASE4_ERROR"], -1, bytes(32)
    terms, secret = [], 0
    for i in range(c.n):
        if c.r[i]:
            xs, ys = [p + 1], [c.share(i, p)]
            for q in c.senders():
                if q != p and keep(q, i):
                    xs.append(q + 1)
                    ys.append(c.share(i, q))
            if len(xs) < c.t:
                return NAMES["INSUFFICIENT"], i, bytes(32)
            secret = (secret + FR.lagrange_at_zero(ys, xs)) % L
        elif i == p or c.q[i]:
            terms.append(c.A0[i])
        else:
            return NAMES["PANIC"], i, bytes(32)
    return NAMES["OK"], -1, FR.gsum(terms + [FR.g_mul(secret)])


def test_per_dealer_disclosures(be, golden):
    c = Cer.of(golden("fault_recon_only_n10_t4.json"))
    assert [i for i in range(c.n) if c.r[i]] == [2, 7] and c.t == 4
    others = [q for q in c.senders() if q != 0]
    for lo, hi in ((7, 2), (2, 7)):  # dealer `hi` at exactly t points, dealer `lo` at t - 1
        keep = lambda q, i: q in (others[:3] if i == hi else others[2:4])  # noqa: E731
        want = finalise_by_pairs(c, 0, keep)
        assert want[:2] == (NAMES["INSUFFICIENT"], lo)
        seats = [(0, j) for j in range(c.n)]
        got = run_seats(be, [c], seats, c.entries(0, c.senders(), keep))
        assert got[0] == want
        assert got == [finalise_by_pairs(c, j, keep) for j in range(c.n)]
    # different sender sets per dealer, both sufficient: two different Lagrange bases in one seat
    keep = lambda q, i: (q + i) % 3 != 0  # noqa: E731
    want = [finalise_by_pairs(c, j, keep) for j in range(c.n)]
    assert {w[0] for w in want} == {NAMES["OK"]}
    assert run_seats(be, [c], [(0, j) for j in range(c.n)], c.entries(0, c.senders(), keep)) == want


# ---------------------------------------------------------------- 4. lane shapes
@pytest.fixture(scope="module")
def wide(be):
    """n = 70, t = 3 from the CPU oracle: dealer 5 reconstructed, everybody qualified."""
    n, t = 70, 3
    h = be.env_init(t, n, CK)
    a, b = dkg_amd.dealer_coefficients(b"\x51" * 32, 0, 0, n, t)
    E, A, s, sp = O.share_gen(n, n, t, a, b, h)
    return Cer(n, t, [1] * n, [int(i == 5) for i in range(n)], A, s)


def test_lane_shapes_wide(be, wide):
    c = wide
    n = c.n
    final = c.senders()
    assert len(final) == 69
    # seat 0 with 62, 63, 64 and 68 listed senders: 63, 64, 65 and 69 points (a lane's second point from 65)
    counts = (62, 63, 64, 68)
    masks = []
    for k, cnt in enumerate(counts):
        listed = random.Random(k).sample([q for q in final if q != 0], cnt)
        masks.append([int(q in listed) for q in range(n)])
    cers = [c] * len(counts)
    entries = [e for g, m in enumerate(masks) for e in c.entries(g, c.senders(m))]
    random.Random(9).shuffle(entries)
    seats = [(g, j) for g in range(len(counts)) for j in (0, 5, 69)]
    got = both(be, lambda: run_seats(be, cers, seats, entries))
    for (g, j), res in zip(seats, got):
        assert res == expect_seat(c, j, masks[g]), (counts[g], j)
        assert res[0] == NAMES["OK"]
    # everybody lists: 69 points for a final seat, 70 for the reconstructed party itself
    got = run_seats(be, [c], [(0, 0), (0, 5)], c.entries(0, final))
    assert got == [expect_seat(c, 0), expect_seat(c, 5)]


def test_lane_shapes_fixtures(be, golden):
    c = golden("ceremony_n64_t31.json")
    w = Cer.of(c, recon=[int(i == 3) for i in range(64)])
    assert w.q == [1] * 64
    seats = [(0, 0), (0, 3), (0, 63)]  # 63 points, 64 (the reconstructed party: every final party is another), 63
    got = both(be, lambda: run_seats(be, [w], seats, w.entries(0, w.senders())))
    assert got == [expect_seat(w, j) for _, j in seats] and {x[0] for x in got} == {0}
    # one point: the empty product, lambda = 1, the secret is the seat's own share
    c3 = golden("ceremony_n3_t1.json")
    w = Cer.of(c3, recon=[0, 1, 0])
    got = run_seats(be, [w], [(0, j) for j in range(3)], [])
    assert got == [expect_seat(w, j, [0, 0, 0]) for j in range(3)] and {x[0] for x in got} == {0}
    assert got[0][2] == FR.gsum([w.A0[0], w.A0[2], FR.g_mul(w.share(1, 0))])
    c2 = golden("ceremony_n2_t0.json")
    w = Cer.of(c2, recon=[0, 1])
    for entries in ([], w.entries(0, w.senders())):
        got = run_seats(be, [w], [(0, 0), (0, 1)], entries)
        d = None if entries else [0, 0]
        assert got == [expect_seat(w, 0, d), expect_seat(w, 1, d)] and {x[0] for x in got} == {0}


# ---------------------------------------------------------------- 5. ignored and rejected input
def test_ignored_and_rejected(be, golden):
    c = Cer.of(golden("fault_recon_only_n10_t4.json"))
    clean = Cer.of(golden("ceremony_n10_t4.json"))
    n, t = c.n, c.t
    cers = [c, clean, c]
    seats = [(0, j) for j in range(n)] + [(1, 4), (1, 0)]  # ceremony 2 is named by nobody
    base = c.entries(0, c.senders())
    want = run_seats(be, cers, seats, base)
    assert want[:n] == [expect_seat(c, j) for j in range(n)] and want[n:] == [expect_seat(clean, 4), expect_seat(clean, 0)]
    junk = bytes(range(32))
    extra = [(0, 3, 3, junk), (0, 8, 8, junk),  # senders that are not final (reconstructed themselves)
             (0, 1, 1, junk), (0, 2, 5, junk),  # dealers that are not reconstructed
             (1, 1, 2, junk),                   # a ceremony without a reconstructed dealer
             (2, 1, 3, junk), (2, 3, 3, junk)]  # a ceremony no seat names
    assert run_seats(be, cers, seats, base + extra) == want
    # sender == the seat's own party is in `base` already for every final seat; without it nothing changes
    own = run_seats(be, cers, seats[:1], [e for e in base if e[1] != 1])
    assert own == want[:1]
    # share + l reads as the share
    plus = [(g, q, i, (int.from_bytes(sh, "little") + L).to_bytes(32, "little")) for g, q, i, sh in base]
    assert run_seats(be, cers, seats, plus) == want
    # rejected
    for bad in (base + base[:1], base + [(0, 0, 3, junk)], base + [(0, n + 1, 3, junk)], base + [(3, 1, 3, junk)],
                base + [(0, 1, 0, junk)], base + [(0, 1, n + 1, junk)]):
        with pytest.raises(DkgError):
            run_seats(be, cers, seats, bad)
    q, r = bytes(x for w in cers for x in w.q), bytearray(x for w in cers for x in w.r)
    qq = bytearray(q)
    qq[2] = 0  # dealer 2 of ceremony 0: reconstructed and not qualified
    with pytest.raises(DkgError):
        run_seats(be, cers, seats, base, sets=(bytes(qq), bytes(r)))
    for g, j in ((0, n), (3, 0)):
        with pytest.raises(DkgError):
            be.finalise_seats(3, n, t, [g], [j], q, bytes(r), b"".join(a for w in cers for a in w.A0), bytes(32 * n))
        with pytest.raises(DkgError):
            be.party_round3_seats(3, n, t, [g], [j], q, bytes(32 * n))
    # the unnamed ceremony: nothing of it is read
    A0 = b"".join(a for w in cers for a in w.A0)
    qq = bytearray(q)
    qq[2 * n + 2] = 0  # reconstruct without qualified there
    assert run_seats(be, cers, seats, base, A0=A0[:32 * 2 * n] + BAD * n, sets=(bytes(qq), bytes(r))) == want
    # a needed A_0 that does not decode or was not fetched: PANIC at that dealer, in index order
    for i in (1, 4):
        bad_a = A0[:32 * i] + BAD + A0[32 * i + 32:]
        f3 = bytes(int(k != i) for k in range(3 * n))
        for got in (run_seats(be, cers, seats, base, A0=bad_a), run_seats(be, cers, seats, base, fetched3=f3)):
            assert got[:n] == [(NAMES["PANIC"], i, bytes(32))] * n and got[n:] == want[n:]
    bad_a = A0[:32 * 4] + BAD + A0[32 * 5:32 * 6] + BAD + A0[32 * 7:]
    assert run_seats(be, cers, seats, base, A0=bad_a)[:n] == [(NAMES["PANIC"], 4, bytes(32))] * n
    # ... on a reconstructed dealer it is never read
    for i in (2, 7):
        bad_a = A0[:32 * i] + BAD + A0[32 * i + 32:]
        f3 = bytes(int(k != i) for k in range(3 * n))
        assert run_seats(be, cers, seats, base, A0=bad_a, fetched3=f3) == want
    # nothing to do
    assert run_seats(be, cers, [], base) == []
    pf = be.finalise_seats(3, n, t, [1], [4], q, bytes(r), A0, seat_cols([w.s for w in cers], n, [(1, 4)]))
    assert (pf.status, pf.recovery_index, pf.mpk) == ([0], [-1], [expect_seat(clean, 4)[2]])
    assert be.party_round3_seats(3, n, t, [], [], q, b"") == (b"", b"")


# ---------------------------------------------------------------- 6. the complaint calls
@pytest.fixture(scope="module")
def three(be, golden):
    """full_faults_n10_t4 with its five round-1 complaints and nine round-4 complaints against dealer 2,
    full_n10_t4 without complaints, and the faulted one again."""
    be.env_init(4, 10, CK)
    c1 = faulted_ceremony(golden)
    c1.pop("shares")
    return [c1, golden_full(golden, "full_n10_t4.json"), dict(c1)]


def flat(cers, key, seed):
    out = [(g, x) for g, c in enumerate(cers) for x in c[key]]
    random.Random(seed).shuffle(out)
    return out


def call2(be, cers, items, fetched1=None, want_qualified=True):
    n, t = cers[0]["n"], cers[0]["t"]
    return be.complaints_verify_ceremonies(
        len(cers), n, t, [g for g, _ in items], [x[0] for _, x in items], [x[1] for _, x in items],
        b"".join(c["pk"] for c in cers), b"".join(c["E"] for c in cers),
        b"".join(enc_of(cers[g % len(cers)]["e1"], cers[g % len(cers)]["ct"], n, x[1] - 1, x[0] - 1) for g, x in items),
        b"".join(x[2] for _, x in items), fetched1, want_qualified)


def single2(be, cers, items, fetched1=None):
    n, t = cers[0]["n"], cers[0]["t"]
    verdict, qualified = [None] * len(items), []
    for g, c in enumerate(cers):
        mine = [k for k, (gg, _) in enumerate(items) if gg == g]
        xs = [items[k][1] for k in mine]
        v, q = be.complaints_verify(n, t, [x[0] for x in xs], [x[1] for x in xs], c["pk"], c["E"],
                                    b"".join(enc_of(c["e1"], c["ct"], n, x[1] - 1, x[0] - 1) for x in xs),
                                    b"".join(x[2] for x in xs), fetched1[g * n:(g + 1) * n] if fetched1 else None)
        for k, vk in zip(mine, v):
            verdict[k] = vk
        qualified += q
    return verdict, qualified


def call4(be, cers, items, qualified=None, fetched3=None):
    n, t = cers[0]["n"], cers[0]["t"]
    return be.complaints3_verify_ceremonies(
        len(cers), n, t, [g for g, _ in items], [x[0] for _, x in items], [x[1] for _, x in items],
        b"".join(x[2] for _, x in items), b"".join(x[3] for _, x in items), b"".join(c["E"] for c in cers),
        b"".join(c["A"] for c in cers), qualified, fetched3)


def single4(be, cers, items, qualified=None, fetched3=None):
    n, t = cers[0]["n"], cers[0]["t"]
    verdict, recon = [None] * len(items), []
    for g, c in enumerate(cers):
        mine = [k for k, (gg, _) in enumerate(items) if gg == g]
        xs = [items[k][1] for k in mine]
        v, r = be.complaints3_verify(n, t, [x[0] for x in xs], [x[1] for x in xs], b"".join(x[2] for x in xs),
                                     b"".join(x[3] for x in xs), c["E"], c["A"],
                                     qualified[g * n:(g + 1) * n] if qualified else None,
                                     fetched3[g * n:(g + 1) * n] if fetched3 else None)
        for k, vk in zip(mine, v):
            verdict[k] = vk
        recon += r
    return verdict, recon


def test_complaint_calls(be, golden, three):
    cers = three
    n = 10
    be.env_init(4, n, CK)
    i2, i4 = flat(cers, "c2", 11), flat(cers, "c4", 12)
    assert len(i2) == 10 and len(i4) == 18
    assert [g for g, _ in i2] != sorted(g for g, _ in i2) and [g for g, _ in i4] != sorted(g for g, _ in i4)  # interleaved
    want2, want4 = single2(be, cers, i2), single4(be, cers, i4)
    assert sorted(want2[0]) == [0] * 6 + [1, 1, 2, 2]
    assert want2[1] == [1, 1, 0, 1, 1, 0, 1, 1, 0, 1] + [1] * n + [1, 1, 0, 1, 1, 0, 1, 1, 0, 1]
    assert want4 == ([0] * 18, [int(i == 1) for i in range(n)] + [0] * n + [int(i == 1) for i in range(n)])
    for mode in (0, 1, 2, 4):
        be.set_complaint_eval(mode)
        assert call2(be, cers, i2) == want2
        assert call4(be, cers, i4) == want4
    be.set_complaint_eval(0)
    assert call2(be, cers, i2, want_qualified=False) == (want2[0], None)
    # the round-3 records of complaints_n10_t4.json over their own ceremony, a clean one and a second copy
    cf = golden("complaints_n10_t4.json")
    p3 = golden(cf["round3_source"])
    plain = [dict(n=n, t=4, E=H(p3["E"]), A=H(p3["A"])), dict(n=n, t=4, E=cers[1]["E"], A=cers[1]["A"])]
    plain.append(plain[0])
    rec = [(x["accuser"], x["accused"], H(x["share"]), H(x["randomness"])) for x in cf["round3"]]
    items = [(0, x) for x in rec] + [(2, x) for x in rec]
    random.Random(13).shuffle(items)
    got = call4(be, plain, items)
    assert got == single4(be, plain, items) and {0} < set(got[0])
    # 63, 64 and 65 complaints in one call
    for cnt in (63, 64, 65):
        items = [(0, x) for x in (cers[0]["c2"] * 13)[:cnt - 2]] + [(2, cers[2]["c2"][0]), (2, cers[2]["c2"][4])]
        assert call2(be, cers, items) == single2(be, cers, items)
        items = [(2, x) for x in (cers[2]["c4"] * 8)[:cnt]]
        assert call4(be, cers, items) == single4(be, cers, items)
    # missing broadcasts and the round-2 set
    f1 = bytes(int(k != 2) for k in range(3 * n))  # dealer 3 of ceremony 0 published no phase-1 broadcast
    got = call2(be, cers, i2, f1)
    assert got == single2(be, cers, i2, f1)
    assert {v for (g, x), v in zip(i2, got[0]) if g == 0 and x[1] == 3} == {COMPLAINT_IGNORED}
    assert got[1][2] == 0 and got[1][2 * n + 2] == 0
    f3 = bytes(int(k != 2 * n + 1) for k in range(3 * n))
    qual = bytes(int(k != 1) for k in range(3 * n))
    got = call4(be, cers, i4, qual, f3)
    assert got == single4(be, cers, i4, qual, f3)
    assert {v for (g, _), v in zip(i4, got[0]) if g == 0} == {COMPLAINT_IGNORED}
    assert {v for (g, _), v in zip(i4, got[0]) if g == 2} == {COMPLAINT_NO_PHASE3}
    assert got[1] == [0] * (2 * n) + [int(i == 1) for i in range(n)]
    # undecodable rows: -1 for a complaint against one, and qualified 0 also where nobody complains
    E0, E1 = cers[0]["E"], cers[1]["E"]
    bad = [dict(cers[0], E=E0[:32 * (5 * 2 + 1)] + BAD + E0[32 * (5 * 2 + 2):]),
           dict(cers[1], E=E1[:32 * 5 * 7] + BAD + E1[32 * 5 * 7 + 32:]), cers[2]]
    got = call2(be, bad, i2)
    assert got == single2(be, bad, i2) and got[1][n + 7] == 0 and got[1][2] == 0
    assert {v for (g, x), v in zip(i2, got[0]) if g == 0 and x[1] == 3} == {-1}
    bad4 = [cers[0], cers[1], dict(cers[2], E=E0[:32 * (5 * 1 + 3)] + BAD + E0[32 * (5 * 1 + 4):])]
    got = call4(be, bad4, i4)
    assert got == single4(be, bad4, i4) and {v for (g, _), v in zip(i4, got[0]) if g == 2} == {-1}
    # nothing to do; arguments
    assert call2(be, cers, []) == ([], [1] * (3 * n))
    assert call4(be, cers, []) == ([], [0] * (3 * n))
    assert be.complaints_verify_ceremonies(0, n, 4, [], [], [], b"", b"", b"", b"") == ([], [])
    with pytest.raises(DkgError):
        call2(be, cers, [(3, cers[0]["c2"][0])])
    with pytest.raises(DkgError):
        call4(be, cers, [(3, cers[0]["c4"][0])])
    with pytest.raises(DkgError):
        call4(be, cers, [(0, (0,) + cers[0]["c4"][0][1:])])


# ---------------------------------------------------------------- 7. the whole path of an operator
def test_whole_path(be, golden, three):
    n, t, B = 10, 4, 4
    N = t + 1
    be.env_init(t, n, CK)
    # a fourth ceremony without round-2 faults whose dealer 2 is reconstructed: its final seats finalise
    f = golden("full_n10_t4.json")
    c3 = golden_full(golden, "full_n10_t4.json")
    c3["A"] = c3["A"][:32 * N] + O.base_mul((321).to_bytes(32, "little")) + c3["A"][32 * N + 32:]
    s, sp = H(f["s"]), H(f["s_prime"])
    c3["c4"] = [(j + 1, 2, s[32 * (n + j):32 * (n + j) + 32], sp[32 * (n + j):32 * (n + j) + 32]) for j in range(n) if j != 1]
    cers = three + [c3]
    ref = dkg_amd.ceremony_batch_verify_full_proven(be, **full_args(cers))
    seats = [(g, j) for g in range(B) for j in range(n)]
    random.Random(21).shuffle(seats)
    cer, js = [g for g, _ in seats], [j for _, j in seats]
    E, A = b"".join(c["E"] for c in cers), b"".join(c["A"] for c in cers)
    col = lambda buf, g, j: b"".join(buf[g][64 * (i * n + j):64 * (i * n + j) + 64] for i in range(n))  # noqa: E731
    e1c = b"".join(col([c["e1"] for c in cers], g, j) for g, j in seats)
    ctc = b"".join(col([c["ct"] for c in cers], g, j) for g, j in seats)
    sks = b"".join(cers[g]["sk"][32 * j:32 * j + 32] for g, j in seats)
    r2 = be.party_round2_seats(B, n, t, cer, js, E, e1c, ctc, sks)
    i2, i4 = flat(cers, "c2", 31), flat(cers, "c4", 32)
    _, qualified = call2(be, cers, i2)
    fs, ps = be.party_round3_seats(B, n, t, cer, js, bytes(qualified), r2["s"])
    dec4 = be.verify_seats(B, n, t, 4, cer, js, A, r2["s"], None, bytes(qualified))
    r4 = [int(1 + sum(1 for i in range(n) if qualified[g * n + i] and dec4[p * n + i] == dkg_amd.ACCEPT) < t + 1)
          for p, (g, j) in enumerate(seats)]
    _, recon = call4(be, cers, i4, bytes(qualified))
    entries = []
    for p, (g, j) in enumerate(seats):
        q, r = qualified[g * n:(g + 1) * n], recon[g * n:(g + 1) * n]
        if not (q[j] and not r[j]) or r2["r2_error"][p] or r4[p]:
            continue  # not a final party, or it never reached Phase4::proceed (:684)
        shares, err = dkg_amd.seat_disclosures(q, r, r2["s"][32 * n * p:32 * n * (p + 1)], t)
        if not err:
            entries += [(g, j + 1, i + 1, sh) for i, sh in enumerate(shares) if sh is not None]
    assert entries
    A0 = b"".join(A[32 * N * k:32 * N * k + 32] for k in range(B * n))
    pf = be.finalise_seats(B, n, t, cer, js, bytes(qualified), bytes(recon), A0, r2["s"], entries,
                           r2_error=r2["r2_error"], r4_error=r4)
    ok = 0
    for g in range(B):
        d = ref.ceremony(g)
        assert qualified[g * n:(g + 1) * n] == list(d["qualified"]) and recon[g * n:(g + 1) * n] == list(d["reconstruct"])
    for p, (g, j) in enumerate(seats):
        d = ref.ceremony(g)
        assert fs[32 * p:32 * p + 32] == d["final_share"][32 * j:32 * j + 32]
        assert ps[32 * p:32 * p + 32] == d["public_share"][32 * j:32 * j + 32]
        assert r4[p] == d["r4_error"][j] and r2["r2_error"][p] == d["r2_error"][j]
        if pf.status[p] == 0 and d["qualified"][j] and not d["reconstruct"][j]:
            assert pf.mpk[p] == d["mpk"], (g, j)
            ok += 1
    # the clean ceremony's ten seats and the nine final seats of the fourth; in the faulted ones every
    # seat meets a disqualified dealer other than itself (committee.rs:791-794)
    assert ok == 19 and sum(recon) == 3
    assert {pf.status[p] for p, (g, _) in enumerate(seats) if g in (0, 2)} == {NAMES["PANIC"]}
    assert {pf.status[p] for p, (g, _) in enumerate(seats) if g in (1, 3)} == {NAMES["OK"]}


# ---------------------------------------------------------------- 8. phase times
def test_phase_times(be, golden):
    c = Cer.of(golden("fault_recon_only_n10_t4.json"))
    try:
        be.set_streams(1)
        run_seats(be, [c], [(0, 0)], c.entries(0, c.senders()))
        ph = be.phase_times("seats")
        assert ph["lagrange"] > 0 and ph["mpk"] > 0
    finally:
        be.set_streams(2)
