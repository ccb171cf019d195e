"""The stepping on a scaled state (dkg_amd/csrc/points.h ge_add_sc_lds, kernels.hip k_stepping<.., SC>)
with the affine normalisations that take its scaled records (k_affine_pairs<SC>, k_affine_pieces<SC>),
and the filtered zero guard of the dedicated additions (fe25519.h fe_zero_guard), at the smallest
shapes that reach each path.

Every decision matrix must equal, byte for byte, the same call under dkg_ctx_set_stepping_formula(1)
(complete additions: there the scaled records are made by a conversion at the store), the UNSPLIT
run of the same committee (U = 1 keeps proper points from the table to the checks: no scaled
record, no folded constant) and, for the tampered dealers, the C oracle's per-pair MSM rows.  Each
shape runs with wrong shares and commitments (no redo) and with an identity E row, whose dedicated
additions are exceptional: the marked workgroups are redone by the complete formula."""
import random

import pytest

import dkg_amd
from dkg_amd import ACCEPT, REJECT, SELF
from tests.test_gpu_stepping_bands import CK, _bump, _check, _committee, _verify

pytestmark = pytest.mark.gpu

P25519 = 2**255 - 19
W = [26 if i % 2 == 0 else 25 for i in range(10)]
P_LIMBS = [0x3ffffed] + [(1 << W[i]) - 1 for i in range(1, 10)]


@pytest.fixture(scope="module")
def be():
    b = dkg_amd.Backend(0)
    yield b
    b.close()


# ---- n = 256, t = 127: one committee, shared by every split ------------------------------------
N256 = (256, 127, 256)


@pytest.fixture(scope="module")
def committee256(be):
    n, t, D = N256
    E, A, s, sp, exp = _committee(be, n, t, D, seed=91)
    ref = _verify(be, n, t, D, E, A, s, sp, 1, formula=1)  # unsplit, complete additions: proper points only
    _check(n, D, ref[0], ref[1], exp, "reference")
    Ei = bytearray(E)
    d = D - 2  # a dealer of the last stepping workgroup
    Ei[32 * d * (t + 1):32 * (d + 1) * (t + 1)] = bytes(32 * (t + 1))
    refi = _verify(be, n, t, D, Ei, A, s, sp, 1, formula=1)
    assert refi[0][d * n:(d + 1) * n] == bytes(SELF if j == d else REJECT for j in range(n))
    return E, Ei, A, s, sp, exp, ref[:2], refi[:2]


# U, slot mode, what the shape reaches
SPLITS = [
    (2, 0),  # pieces of 64, four segments per workgroup, banded map; k_affine_pairs takes the scaled records
    (4, 2),  # pieces of 32, eight segments per workgroup (per-piece tables)
    (4, 1),  # the four pieces of a column in one slot
    (3, 0),  # 43 + 43 + 42: ragged last piece, contiguous map; k_affine_pieces with the dense Z copy
    (1, 0),  # the checks read R: proper points, the dedicated loop keeps its doublings (tail phases)
]


@pytest.mark.parametrize("U,mode", SPLITS)
def test_scaled_stepping_matches_complete_and_unsplit(be, committee256, U, mode):
    n, t, D = N256
    E, Ei, A, s, sp, exp, ref, refi = committee256
    d2, d4, r2, r4 = _verify(be, n, t, D, E, A, s, sp, U, stepping=mode)
    assert (r2, r4) == (0, 0)  # wrong shares and commitments are no exceptional pairs
    _check(n, D, d2, d4, exp, (U, mode))
    assert (d2, d4) == ref
    c2, c4, q2, q4 = _verify(be, n, t, D, E, A, s, sp, U, stepping=mode, formula=1)
    assert (c2, c4) == (d2, d4) and (q2, q4) == (0, 0)
    # the identity E row: redone workgroups, the same decisions
    x2, x4, r2, r4 = _verify(be, n, t, D, Ei, A, s, sp, U, stepping=mode)
    assert r2 > 0 and r4 == 0
    assert (x2, x4) == refi
    c2, c4, q2, q4 = _verify(be, n, t, D, Ei, A, s, sp, U, stepping=mode, formula=1)
    assert (c2, c4) == (x2, x4) and (q2, q4) == (0, 0)


# ---- a piece of more than 512 positions: the block launches' up / down streams ------------------
def test_scaled_streams_of_multiblock_pieces(be):
    """t + 1 = 1030 at U = 2: pieces of 515 positions in two 258-lane blocks each, the upper block
    streaming its scaled cached form down (the smallest split table the drivers chain through
    streams).  Four dealers, one with wrong shares, one with an identity E row; a pair verification
    needs no t < (n + 1) / 2."""
    n, t, D = 1040, 1029, 4
    N = t + 1
    be.env_init(1, n, CK)
    a, b = dkg_amd.dealer_coefficients(b"\x2f" * 32, 5, 0, D, t)
    E, A, s, sp = (bytearray(x) for x in be.share_gen(a, b, D, n, t))
    for j in (1, 257, 258, n - 1):  # receivers whose values cross the block boundary at different steps
        _bump(s, 32 * (0 * n + j))
    ref = _verify(be, n, t, D, E, A, s, sp, 1, formula=1)
    row = lambda m, i: m[i * n:(i + 1) * n]  # noqa: E731
    assert row(ref[0], 0).count(REJECT) == 4 and row(ref[1], 0).count(REJECT) == 4
    assert all(row(m, i) == bytes(SELF if j == i else ACCEPT for j in range(n)) for m in ref[:2] for i in (1, 2, 3))
    d2, d4, r2, r4 = _verify(be, n, t, D, E, A, s, sp, 2)
    assert be.last_split_len() == 515 and (r2, r4) == (0, 0)
    assert (d2, d4) == ref[:2]
    assert _verify(be, n, t, D, E, A, s, sp, 2, formula=1)[:2] == (d2, d4)
    E[32 * 2 * N:32 * 3 * N] = bytes(32 * N)
    x2, x4, r2, r4 = _verify(be, n, t, D, E, A, s, sp, 2)
    assert r2 > 0 and r4 == 0
    assert row(x2, 2) == bytes(SELF if j == 2 else REJECT for j in range(n))
    assert (x2, x4) == _verify(be, n, t, D, E, A, s, sp, 1, formula=1)[:2]
    assert (x2, x4) == _verify(be, n, t, D, E, A, s, sp, 2, formula=1)[:2]


# ---- n = 64, t = 31, a batch: the tail phases' compact states stay proper ------------------------
def test_batch_tail_phases_with_filtered_guard(be, golden):
    """Three n = 64, t = 31 ceremonies in one batch (the dead-position repack: unsplit tables, proper
    points in the compact states, the filtered guard in every phase): the honest fixture, the same
    with a wrong share, and one with an identity E row; then the single ceremonies, also on the
    per-step binomial without lane pairs, whose guard makes the driver rerun the verification."""
    g = golden("ceremony_n64_t31.json")
    n, t = 64, 31
    N = t + 1
    H = bytes.fromhex
    be.env_init(t, n, CK)
    E, A, s, sp = H(g["E"]), H(g["A"]), H(g["s"]), H(g["s_prime"])
    s1 = bytearray(s)
    _bump(s1, 32 * (5 * n + 9))
    E2 = bytearray(E)
    E2[32 * N * 7:32 * N * 8] = bytes(32 * N)
    args = (E + E + bytes(E2), A * 3, s + bytes(s1) + s, sp * 3)
    outs = []
    try:
        for formula in (0, 1):
            be.set_stepping_formula(formula)
            r = dkg_amd.ceremony_batch_verify(be, 3, n, t, *args)
            outs.append([r.ceremony(c) for c in range(3)])
    finally:
        be.set_stepping_formula(0)
    for c in range(3):
        for k in ("dec2", "dec4", "qualified", "reconstruct", "final_share", "mpk"):
            assert outs[0][c][k] == outs[1][c][k], (c, k)
    d = outs[0][0]
    assert "".join(str(x) for x in d["dec2"]) == g["dec2"] and "".join(str(x) for x in d["dec4"]) == g["dec4"]
    assert d["final_share"].hex() == g["final_share"] and d["mpk"].hex() == g["mpk"]
    assert bytes(outs[0][1]["dec2"])[5 * n:6 * n].count(REJECT) == 1
    assert bytes(outs[0][2]["dec2"])[7 * n:8 * n] == bytes(SELF if j == 7 else REJECT for j in range(n))
    # the single ceremony with the identity row: its tail phases' marked workgroups are redone (at this
    # size every binomial step runs on lane pairs, which use the complete formula: no rerun)
    r = be.ceremony_verify(bytes(E2), A, s, sp, n, t)
    assert be.stepping_redos() > 0 and be.binomial_reruns() == 0
    assert bytes(r.dec2) == bytes(outs[0][2]["dec2"]) and bytes(r.dec4) == bytes(outs[0][2]["dec4"])
    # without lane pairs the steps run the dedicated chain with the filtered guard: it marks the guard
    # word, and the driver reruns the verification with the complete formula
    be.set_binomial(1)
    try:
        r1 = be.ceremony_verify(bytes(E2), A, s, sp, n, t)
        assert be.binomial_reruns() == 1
        assert (r1.dec2, r1.dec4, r1.mpk) == (r.dec2, r.dec4, r.mpk)
        r1 = be.ceremony_verify(E, A, bytes(s1), sp, n, t)
        assert be.binomial_reruns() == 0 and be.stepping_redos() == 0
    finally:
        be.set_binomial(0)
    r = be.ceremony_verify(E, A, bytes(s1), sp, n, t)
    assert be.binomial_reruns() == 0 and be.stepping_redos() == 0
    assert bytes(r.dec2) == bytes(outs[0][1]["dec2"])


# ---- the filter and the full test on chosen limbs ------------------------------------------------
def _limbs(x):
    out = []
    for w in W:
        out.append(x & ((1 << w) - 1))
        x >>= w
    return out


def test_zero_guard_equals_full_test(be):
    """dkg_zero_tests on all-zero limbs, p's limbs, p's limbs with one other limb changed, random
    tight values whose limb 9 is 0 or 2^25 - 1 (the filter fires, the full test decides) and random
    tight values: the filtered guard equals fe_tight_zero on every one, the filter is necessary for
    it, and the full test is true exactly on the two representations of zero."""
    rng = random.Random(25519)
    cases = [[0] * 10, list(P_LIMBS)]
    for i in range(10):
        for delta in (1, -1):
            v = list(P_LIMBS)
            v[i] = (v[i] + delta) & 0xffffffff if i != 9 or delta < 0 else 0
            cases.append(v)
        z = [0] * 10
        z[i] = 1
        cases.append(z)
    for _ in range(40):
        v = _limbs(rng.randrange(P25519))
        v[9] = rng.choice((0, 0x1ffffff))
        cases.append(v)
    # tight means limbs 1 and 5 may exceed their width by a small carry (fe25519.h)
    for _ in range(40):
        v = _limbs(rng.randrange(P25519))
        v[1] += rng.randrange(1 << 11)
        v[5] += rng.randrange(1 << 11)
        cases.append(v)
    # a filter hit in one lane must not change the other lanes of its wave: mixed waves of 64
    cases += [_limbs(rng.randrange(P25519)) for _ in range(150 - len(cases) % 64)]
    res = be.zero_tests(cases)
    assert len(res) == len(cases)
    for v, (filt, full, guard) in zip(cases, res):
        zero = v == [0] * 10 or v == P_LIMBS
        assert full == (1 if zero else 0), v
        assert guard == full, v
        assert filt == (1 if v[9] in (0, 0x1ffffff) else 0), v
        assert filt >= full, v
    assert sum(f for f, _, _ in res) >= 42 and sum(f for _, f, _ in res) == 2
