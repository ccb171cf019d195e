"""dkg_seat_finalise_status and seat_disclosures (host only, no GPU): the status rule dkg_finalise_seats
executes per seat, against tests/finalise_ref.py party_finalise on the libsodium fixtures and on random
draws, and Phases<Phase4>::proceed's per-seat output against the fixtures' reconstruct."""
import random

import pytest

import dkg_amd
from dkg_amd import DkgError
from tests import finalise_ref as FR

H = bytes.fromhex
NAMES = {"OK": 0, "R2_ERROR": 1, "R4_ERROR": 2, "PHASE4_ERROR": 3, "INSUFFICIENT": 4, "PANIC": 5}
A0 = [bytes(32)] * 24  # the identity: party_finalise sums them, the status does not depend on them


def points_held(p, n, qualified, recon, disclosed=None, r2_error=None, r4_error=None):
    """What party p holds for every reconstructed dealer under party_finalise's sender rule: its own
    share plus the disclosures of the other final parties without an earlier failure."""
    cnt = 1 + sum(1 for q in range(n)
                  if q != p and (disclosed is None or disclosed[q]) and qualified[q] and not recon[q]
                  and not (r2_error and r2_error[q]) and not (r4_error and r4_error[q]))
    return [cnt] * n


def ref_status(p, n, t, qualified, recon, points, a_present=None, r2=False, r4=False):
    """party_finalise's loop (committee.rs:745-797) with the points held given per dealer and the rule of
    dkg_ceremony_verify_fetched_proven for a qualified dealer without a usable phase-3 broadcast."""
    if r2:
        return "R2_ERROR", -1
    if r4:
        return "R4_ERROR", -1
    if sum(qualified) - sum(recon) <= t:
        return "PHASE4_ERROR", -1
    for i in range(n):
        if recon[i]:
            if points[i] < t:
                return "INSUFFICIENT", i
        elif not qualified[i]:
            if i != p:
                return "PANIC", i
        elif a_present is not None and not a_present[i]:
            return "PANIC", i
    return "OK", -1


@pytest.mark.parametrize("name", ["finalise_parties_n10_t4.json", "finalise_parties_recon_n10_t4.json"])
def test_fixture_cases(golden, name):
    f = golden(name)
    c = golden(f["source"])
    n, t = c["n"], c["t"]
    q, r = [int(x) for x in c["qualified"]], [int(x) for x in c["reconstruct"]]
    for case in f["cases"]:
        d, r2, r4 = case.get("disclosed"), case.get("r2_error"), case.get("r4_error")
        for p in range(n):
            pts = points_held(p, n, q, r, d, r2, r4)
            st, idx, _ = FR.party_finalise(p, n, t, q, r, A0, lambda i, j: 1, disclosed=d, r2_error=r2, r4_error=r4)
            assert (st, idx) == (case["status"][p], case["index"][p])
            got = dkg_amd.seat_finalise_status(n, t, p, q, r, pts, None, bool(r2 and r2[p]), bool(r4 and r4[p]))
            assert got == (NAMES[st], idx), (case["name"], p)
            assert ref_status(p, n, t, q, r, pts, None, r2 and r2[p], r4 and r4[p]) == (st, idx)


def test_phase4_error_fixture(golden):
    c = golden("fault_a_many_n10_t4.json")
    n, t = c["n"], c["t"]
    q, r = [int(x) for x in c["qualified"]], [int(x) for x in c["reconstruct"]]
    assert c["phase4_error"]
    for p in range(n):
        assert dkg_amd.seat_finalise_status(n, t, p, q, r, [n] * n) == (NAMES["PHASE4_ERROR"], -1)
        assert FR.party_finalise(p, n, t, q, r, A0, lambda i, j: 1)[:2] == ("PHASE4_ERROR", -1)
        # the seat's own earlier failures come first
        assert dkg_amd.seat_finalise_status(n, t, p, q, r, [n] * n, r4_error=True) == (NAMES["R4_ERROR"], -1)
        assert dkg_amd.seat_finalise_status(n, t, p, q, r, [n] * n, r2_error=True, r4_error=True) == (NAMES["R2_ERROR"], -1)
        assert dkg_amd.seat_disclosures(q, r, H(c["s"])[:32 * n], t) == (None, True)


def test_random_draws():
    rng = random.Random(77)
    seen = set()
    for _ in range(600):
        n = rng.randint(1, 24)
        t = rng.randint(0, (n - 1) // 2)
        q = [int(rng.random() < 0.85) for _ in range(n)]
        r = [int(q[i] and rng.random() < 0.25) for i in range(n)]
        pts = [rng.choice([0, 1, max(t - 1, 0), t, t + 1, n]) for _ in range(n)]
        ap = None if rng.random() < 0.3 else [int(rng.random() < 0.9) for _ in range(n)]
        r2, r4 = rng.random() < 0.05, rng.random() < 0.05
        p = rng.randrange(n)
        want = ref_status(p, n, t, q, r, pts, ap, r2, r4)
        assert dkg_amd.seat_finalise_status(n, t, p, q, r, pts, ap, r2, r4) == (NAMES[want[0]], want[1]), (n, t, q, r, pts)
        seen.add(want[0])
        # where every dealer holds the same count and every A_0 is present, the rule is party_finalise's
        if ap is None and not r2 and not r4:
            d = [int(rng.random() < 0.6) for _ in range(n)]
            held = points_held(p, n, q, r, d)
            st, idx, _ = FR.party_finalise(p, n, t, q, r, A0, lambda i, j: 1, disclosed=d)
            assert dkg_amd.seat_finalise_status(n, t, p, q, r, held) == (NAMES[st], idx)
    assert seen == set(NAMES)


def test_arguments():
    with pytest.raises(DkgError):
        dkg_amd.seat_finalise_status(3, 1, 3, [1, 1, 1], [0, 0, 0], [1, 1, 1])  # p >= n
    with pytest.raises(DkgError):
        dkg_amd.seat_finalise_status(3, 1, 0, [1, 0, 1], [0, 1, 0], [1, 1, 1])  # reconstruct without qualified
    with pytest.raises(DkgError):
        dkg_amd.seat_finalise_status(0, 0, 0, [], [], [])


@pytest.mark.parametrize("name", ["fault_recon_only_n10_t4.json", "fault_self_share_n10_t4.json", "full_n10_t4.json",
                                  "fault_share_flip_n10_t4.json"])
def test_seat_disclosures(golden, name):
    c = golden(name)
    n, t = c["n"], c["t"]
    s = H(c["s"])
    q, r = [int(x) for x in c["qualified"]], [int(x) for x in c["reconstruct"]]
    for j in range(n):
        col = b"".join(s[32 * (i * n + j):32 * (i * n + j) + 32] for i in range(n))
        shares, err = dkg_amd.seat_disclosures(q, r, col, t)
        assert err == bool(c["phase4_error"])
        if err:
            assert shares is None
            continue
        assert [x is not None for x in shares] == [bool(x) for x in r]
        assert all(x == col[32 * i:32 * i + 32] for i, x in enumerate(shares) if x is not None)
        assert dkg_amd.seat_disclosures(q, r, col) == (shares, None)  # without t: no phase4_error
    with pytest.raises(ValueError):
        dkg_amd.seat_disclosures([1, 0], [0, 1], bytes(64), 0)
