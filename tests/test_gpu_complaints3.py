"""Round-4 complaints on the GPU (complaints.hip k_c3_*): MisbehavingPartiesRound3::verify
(broadcast.rs:104-144) as Phases<Phase4>::proceed applies it (committee.rs:636-670), one lane per complaint.

Expected values come from the CPU oracle (tests/oracle_lib.py complaint3_verify, share_gen) and the
libsodium fixtures; the host-driven primitive Backend.complaint3_verify is the second opinion.
Bit-exact throughout.
"""
import random

import pytest

import dkg_amd
from dkg_amd import COMPLAINT_IGNORED, COMPLAINT_NO_PHASE3
from tests import oracle_lib as O
from tests.test_oracle import VERDICT

pytestmark = pytest.mark.gpu

H = bytes.fromhex
L = 2**252 + 27742317777372353535851937790883648493
CK = b"Example of a shared string."
G = H("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76")


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
    """What receiver q (0-based) decrypted from dealer i: (share, randomness)."""
    k = 32 * (i * n + q)
    return s[k:k + 32], sp[k:k + 32]


def bad_coefficient(C, N, i, k, point):
    C = bytearray(C)
    C[32 * (N * i + k):32 * (N * i + k + 1)] = point
    return bytes(C)


def oracle(h, t, N, E, A, comp):
    """comp: [(accuser, accused, share, randomness)], 1-based."""
    return [O.complaint3_verify(h, t, q, sh, rn, row(E, N, i - 1), row(A, N, i - 1)) for q, i, sh, rn in comp]


def run(be, n, t, comp, E, A, qualified=None, fetched3=None):
    return be.complaints3_verify(n, t, [c[0] for c in comp], [c[1] for c in comp], b"".join(c[2] for c in comp),
                                 b"".join(c[3] for c in comp), E, A, qualified, fetched3)


# ---------------- 1. fixture ----------------
def test_fixture(be, golden):
    """The eleven round3 records of complaints_n10_t4.json over fault_a_generator_n10_t4.json: nine valid
    complaints against dealer 6, the honest pair (FalseClaimedInequality), the share + 1
    (FalseClaimedEquality), in every evaluation mode."""
    c = golden("complaints_n10_t4.json")
    p3 = golden(c["round3_source"])
    n, t = p3["n"], p3["t"]
    N = t + 1
    assert p3["h"] == be.env_init(t, n, CK).hex()
    E, A = H(p3["E"]), H(p3["A"])
    comp = [(x["accuser"], x["accused"], H(x["share"]), H(x["randomness"])) for x in c["round3"]]
    exp = [VERDICT[x["verdict"]] for x in c["round3"]]
    assert exp == [0] * 9 + [2, 3]
    second = be.complaint3_verify(t, [x[0] for x in comp], b"".join(x[2] for x in comp), b"".join(x[3] for x in comp),
                                  b"".join(row(E, N, x[1] - 1) for x in comp),
                                  b"".join(row(A, N, x[1] - 1) for x in comp))
    assert second == exp
    for mode in (0, 1, 2):
        be.set_complaint_eval(mode)
        v, rec = run(be, n, t, comp, E, A)
        assert v == exp, mode
        assert rec == [int(i == 5) for i in range(n)] == p3["reconstruct"], mode
    be.set_complaint_eval(0)


# ---------------- 2. random batch against the oracle ----------------
CHEATS = [2, 5, 11, 17, 23, 31, 38]
NO_PHASE3, BAD_A, DISQUALIFIED, BAD_E = 8, 14, 20, 27


@pytest.fixture(scope="module")
def batch(be):
    """n = 40, t = 19: seven dealers with one A coefficient replaced by another valid point, each accused by
    all 39 others with the pair they hold (273 complaints: past a 256-lane workgroup and into a fifth
    wave), plus the odd ones.  Inputs and oracle verdicts, computed once."""
    rng = random.Random(4242)
    n, t = 40, 19
    N = t + 1
    h = be.env_init(t, n, CK)
    a, b = dkg_amd.dealer_coefficients(b"\x71" * 32, 0, 0, n, t)
    E, A, s, sp = O.share_gen(n, n, t, a, b, h)
    for i in CHEATS:
        A = bad_coefficient(A, N, i, rng.randrange(N), O.base_mul(sc(1000 + i)))
    A = bad_coefficient(A, N, BAD_A, 7, b"\xff" * 32)
    E = bad_coefficient(E, N, BAD_E, 3, b"\xff" * 32)
    qualified = bytearray([1] * n)
    qualified[DISQUALIFIED] = 0
    fetched3 = bytearray([1] * n)
    fetched3[NO_PHASE3] = 0

    def true(i, q):
        return (q + 1, i + 1) + pair(s, sp, n, i, q)

    def plus1(x):
        return sc(int.from_bytes(x, "little") + 1)

    comp = [true(i, q) for i in CHEATS for q in range(n) if q != i]
    assert len(comp) == 273
    q, i, sh, rn = true(2, 3)
    comp.append((q, i, plus1(sh), rn))                                # share + 1
    comp.append((q, i, sh, plus1(rn)))                                # randomness + 1
    comp.append(true(0, 6))                                           # an honest pair: dealer 1 is honest
    comp.append(true(11, 8))                                          # (9, 12) again
    comp.append((3, NO_PHASE3 + 1, sc(rng.randrange(L)), sc(rng.randrange(L))))  # no phase-3 broadcast, garbage
    comp.append(true(BAD_A, 1))                                       # an A coefficient that does not decode
    comp.append(true(DISQUALIFIED, 4))                                # a disqualified accused
    comp.append(true(BAD_E, 5))                                       # an E coefficient that does not decode
    return dict(n=n, t=t, N=N, h=h, E=E, A=A, s=s, sp=sp, comp=comp, qualified=bytes(qualified),
                fetched3=bytes(fetched3), oracle=oracle(h, t, N, E, A, comp))


def test_batch_oracle_is_as_intended(batch):
    o = batch["oracle"]
    assert o[:273] == [0] * 273
    # the oracle knows no fetched3 / qualified: garbage scalars fail the E side, the honest pair of the
    # disqualified (honest) dealer is a false claim, undecodable rows are -1
    assert o[273:] == [3, 3, 2, 0, 3, -1, 2, -1]


EXPECTED_TAIL = [3, 3, 2, 0, COMPLAINT_NO_PHASE3, COMPLAINT_NO_PHASE3, COMPLAINT_IGNORED, -1]


@pytest.mark.parametrize("mode", [1, 2, 0])
def test_batch_against_oracle(be, batch, mode):
    d = batch
    n = d["n"]
    be.env_init(d["t"], n, CK)
    be.set_complaint_eval(mode)
    v, rec = run(be, n, d["t"], d["comp"], d["E"], d["A"], d["qualified"], d["fetched3"])
    be.set_complaint_eval(0)
    assert v == d["oracle"][:273] + EXPECTED_TAIL
    assert rec == [int(i in CHEATS + [NO_PHASE3, BAD_A]) for i in range(n)]


def test_batch_defaults_and_noncanonical(be, batch):
    """qualified / fetched3 = NULL read as all 1; scalar bytes beyond the canonical range (share + l, and the
    same with bit 255 set) are read as the host-driven primitive reads them."""
    d = batch
    n, t, N = d["n"], d["t"], d["N"]
    be.env_init(t, n, CK)
    tail = d["comp"][273:]
    v, rec = run(be, n, t, tail, d["E"], d["A"])
    assert v == [3, 3, 2, 0, 3, COMPLAINT_NO_PHASE3, 2, -1]
    assert rec == [int(i in (11, BAD_A)) for i in range(n)]
    q, i, sh, rn = d["comp"][0]
    big = int.from_bytes(sh, "little") + L
    odd = [(q, i, big.to_bytes(32, "little"), rn), (q, i, (big | 1 << 255).to_bytes(32, "little"), rn),
           (q, i, sh, (int.from_bytes(rn, "little") | 1 << 255).to_bytes(32, "little"))]
    second = be.complaint3_verify(t, [q] * 3, b"".join(x[2] for x in odd), b"".join(x[3] for x in odd),
                                  row(d["E"], N, i - 1) * 3, row(d["A"], N, i - 1) * 3)
    for mode in (1, 2):
        be.set_complaint_eval(mode)
        assert run(be, n, t, odd, d["E"], d["A"])[0] == second, mode
    be.set_complaint_eval(0)


# ---------------- 3. the automatic mode mixes both paths ----------------
def test_automatic_mode_mixes_both_paths(be):
    """n = 130, t = 12, the shapes of test_gpu_complaints.test_automatic_mode_mixes_both_paths (chain
    arithmetic there): dealer 1, accused by all 129 others, takes the difference tables for both of its
    rows; dealer 7, accused by one, and the false complaint against dealer 4 take Horner walks, in one call."""
    n, t = 130, 12
    N = t + 1
    h = be.env_init(t, n, CK)
    a, b = dkg_amd.dealer_coefficients(b"\x72" * 32, 0, 0, n, t)
    E, A, s, sp = O.share_gen(n, n, t, a, b, h)
    A = bad_coefficient(A, N, 0, 5, O.base_mul(sc(77)))
    A = bad_coefficient(A, N, 6, 0, O.base_mul(sc(78)))
    pairs = [(0, q) for q in range(1, n)] + [(6, 99), (3, 4)]
    comp = [(q + 1, i + 1) + pair(s, sp, n, i, q) for i, q in pairs]
    exp = oracle(h, t, N, E, A, comp)
    assert exp == [0] * 130 + [2]
    for mode in (0, 1, 2):
        be.set_complaint_eval(mode)
        v, rec = run(be, n, t, comp, E, A)
        assert v == exp, mode
        assert rec == [int(i in (0, 6)) for i in range(n)], mode
    be.set_complaint_eval(0)


# ---------------- 4. the smallest committees ----------------
@pytest.mark.parametrize("n,t,cheat", [(2, 0, [(0, 1)]), (3, 1, [(2, 0), (1, 0)]), (5, 2, [(4, 1)])])
def test_small_committees(be, n, t, cheat):
    """A constant polynomial (t = 0: the tables cannot run), t = 1, C = 1 and C = 0."""
    N = t + 1
    h = be.env_init(t, n, CK)
    a, b = dkg_amd.dealer_coefficients(b"\x73" * 32, 0, 0, n, t)
    E, A, s, sp = O.share_gen(n, n, t, a, b, h)
    for i, _ in cheat:
        A = bad_coefficient(A, N, i, t, O.base_mul(sc(90 + i)))
    comp = [(q + 1, i + 1) + pair(s, sp, n, i, q) for i, q in cheat]
    false = (1, 2) + pair(s, sp, n, 1, 0) if (1, 0) not in cheat else (2, 1) + pair(s, sp, n, 0, 1)
    exp = oracle(h, t, N, E, A, comp + [false])
    assert exp == [0] * len(cheat) + [2]
    for mode in (0, 1, 2):
        be.set_complaint_eval(mode)
        v, rec = run(be, n, t, comp + [false], E, A)
        assert v == exp, mode
        assert rec == [int(i in [d for d, _ in cheat]) for i in range(n)], mode
        v, rec = run(be, n, t, comp[:1], E, A)
        assert v == [0] and rec == [int(i == cheat[0][0]) for i in range(n)], mode
        assert run(be, n, t, [], E, A) == ([], [0] * n), mode
    be.set_complaint_eval(0)


# ---------------- 5. index width ----------------
def test_accuser_index_13_bits(be):
    """Accusers 4095 (all twelve low bits) and 4096 (only bit 12) at n = 4096, t = 3: the index walk of the
    Horner path and the last table positions.  E and A are 512 KB each: dealer 1's rows real, the rest the
    generator."""
    n, t = 4096, 3
    N = t + 1
    h = be.env_init(t, n, CK)
    a, b = dkg_amd.dealer_coefficients(b"\x74" * 32, 0, 0, 1, t)
    E1, A1, s, sp = O.share_gen(1, n, t, a, b, h)
    rest = G * (N * (n - 1))
    E, A = E1 + rest, A1 + rest
    Abad = bad_coefficient(A1, N, 0, 2, O.base_mul(sc(9))) + rest
    comp = [(j, 1) + pair(s, sp, n, 0, j - 1) for j in (4095, 4096)]
    assert oracle(h, t, N, E, Abad, comp) == [0, 0]
    assert oracle(h, t, N, E, A, comp[1:]) == [2]
    for mode in (1, 2):
        be.set_complaint_eval(mode)
        assert run(be, n, t, comp, E, Abad) == ([0, 0], [1] + [0] * (n - 1)), mode
        assert run(be, n, t, comp[1:], E, A) == ([2], [0] * n), mode  # a false complaint by 4096
    be.set_complaint_eval(0)


# ---------------- 6. arguments ----------------
def test_index_range_env_and_empty(be):
    n, t = 3, 1
    h = be.env_init(t, n, CK)
    a, b = dkg_amd.dealer_coefficients(b"\x75" * 32, 0, 0, n, t)
    E, A, s, sp = O.share_gen(n, n, t, a, b, h)
    sh, rn = pair(s, sp, n, 2, 0)
    for acc, acd in [(0, 3), (4, 3), (1, 0), (1, 4)]:
        with pytest.raises(dkg_amd.DkgError) as e:
            run(be, n, t, [(acc, acd, sh, rn)], E, A)
        assert e.value.code == -1
    assert run(be, n, t, [], E, A) == ([], [0] * n)
    assert run(be, n, t, [], E, A, bytes([1, 0, 1]), bytes([0, 1, 1])) == ([], [0] * n)
    fresh = dkg_amd.Backend(0)
    try:
        with pytest.raises(dkg_amd.DkgError) as e:
            run(fresh, n, t, [(1, 3, sh, rn)], E, A)
        assert e.value.code == -1
    finally:
        fresh.close()
