"""The dedicated additions of the stepping (kernels.hip k_stepping) and of the binomial Horner
(k_binom_step, k_binom_wave) on crafted NON-IDENTITY exceptional pairs: one dealer's coefficients are
solved (tests/crafted_pairs.py) so that two neighbouring table entries are equal -- or opposite -- as
group elements at ONE position and ONE step, with everything before and around them clean.  The two
entries reach the addition through different chains, so their limbs differ: F = B - A is a non-zero
multiple of p (4-torsion offset O or T2), or G = B + A is (an offset of order 4).

Every case takes honest dealers, replaces a few by crafted ones, asserts their commitments equal the
C oracle's, bumps one share of each crafted dealer, and compares the decision rows byte for byte
with the oracle's per-pair MSM rows (never with the code under test), with the same call under the
complete formula (dkg_ctx_set_stepping_formula 1) and with the unsplit complete run.  The redo
counter must be > 0 (an exact count where the launch shape gives one) and 0 for the control: the same
committee with every solved coefficient incremented by one.

tests/test_crafted_pairs.py checks on the CPU that the seeds below give the torsion classes stated
next to them and that the oracle accepts the crafted rows."""
import pytest

import dkg_amd
from dkg_amd import ACCEPT, REJECT, SELF, _lib
from tests import crafted_pairs as CP
from tests import oracle_lib as O
from tests.test_gpu_stepping_bands import CK, _bump, _check, _verify

pytestmark = pytest.mark.gpu

# ---- the committed seeds (crafted_row's seed), with the classes tests/test_crafted_pairs.py asserts
# n = 64, t = 31, unsplit.  seed, m, j, class of the E pair, class of the A pair
STEP_SEEDS = [
    (0, 5, 10, "O", "O"),     # m >= 4: always the same point in two representations, F = 0
    (9, 1, 30, "T2", "T2"),   # F = 0 across the 2-torsion point
    (0, 1, 30, "T4", "T4"),   # G = 0
    (0, 2, 20, "T2", "O"),
]
# dealer: (seed, m, j, E class, A class) of shape 1's committee, n = 64 receivers and 64 dealers
SHAPE1 = {
    0: (0, 5, 10, "O", "O"),      # phase 0 (steps 0..48 on 32 positions)
    63: (1, 1, 58, "T4", "T2"),   # only in phase 2 (steps 57..60 on 8 positions)
    37: (5, 0, 62, "T4", "T2"),   # only in phase 3 (steps 61..63 on 4 positions)
    21: (9, 1, 30, "T2", "T2"),
}
# the same with n = 70 receivers and 70 dealers (phases from steps 0, 55, 63, 67): dealers 64..69 sit in a
# ragged group with 58 padding columns, 63 | 64 are the two sides of a group boundary
SHAPE1R = {
    0: (0, 5, 10, "O", "O"),      # phase 0
    63: (0, 1, 64, "T4", "T2"),   # only in phase 2 (steps 63..66); last column of group 0
    64: (4, 0, 68, "T4", "T2"),   # only in phase 3 (steps 67..69); first column of group 1
    69: (9, 1, 30, "T2", "T2"),   # the last real column
}
# opposite pairs at m = 0: Q(j) = -Delta Q(j), so Q(j + 1) is a pure torsion point.  seed, m, j, class of
# the E sum, class of the A sum (T4: a representative of the identity with Y = 0)
OPP_SEEDS = [(1, 0, 20, "O", "T4"), (0, 0, 20, "T2", "T4"), (7, 0, 20, "T4", "O")]
# binomial, n = 64, t = 31, unsplit: seed, r, m, sign, E class, A class, rerun expected (the model of
# the item: crafted_pairs.binomial_item_meets_zero)
BINOM_SEEDS = [
    (0, 20, 7, +1, "O", "O", True),
    (0, 20, 1, +1, "T4", "T4", True),   # e_0 = e_1 across an order-4 offset: G = 0
    (5, 20, 1, +1, "T2", "T2", True),
    (0, 20, 7, -1, "O", "O", True),     # the sum is the identity; the 7-chain's additions O + O meet Z = 0
    (5, 12, 4, -1, "T2", "T2", False),  # the sum is T2; m = 4 is doublings only: nothing flags
]
# per-wave binomial under a forced 2-way split (pieces of 16): seed, piece, r, m
WAVE_SEEDS = [(0, 1, 10, 4), (1, 1, 10, 1)]
# the batch's crafted dealer: one binomial pair and one stepping pair of a late tail phase
BATCH_ROW = dict(seed=3, binom=[(0, 20, 7)], pairs=[(0, 1, 58)])


@pytest.fixture(scope="module")
def be():
    b = dkg_amd.Backend(0)
    yield b
    b.close()


def _plen(n, t, D, U):
    return t + 1 if U == 1 else _lib.lib().dkg_split_len((D + 63) // 64 * 64, n, t, U)


def _put(buf, N, d, coeffs):
    buf[32 * N * d:32 * N * (d + 1)] = CP.sc_bytes(coeffs)


def crafted_coefficients(n, t, D, seed, rows, plen, sign=+1, control=False):
    """(a, b) of D dealers: dealer_coefficients' honest ones with the dealers of `rows` = {dealer:
    dict(seed, pairs, binom)} replaced by crafted_row's."""
    N = t + 1
    a, b = (bytearray(x) for x in dkg_amd.dealer_coefficients(bytes([seed]) * 32, 5, 0, D, t))
    for d, row in rows.items():
        ca, cb = CP.crafted_row(row["seed"], N, plen, row.get("pairs", []), sign, control, row.get("binom", ()))
        _put(a, N, d, ca)
        _put(b, N, d, cb)
    return bytes(a), bytes(b)


def _committee(be, n, t, D, seed, rows, plen, sign=+1, control=False, bump=None, oracle=True):
    """Broadcasts of that committee, one share of every crafted dealer bumped (receiver bump[d], by
    default (d + 7) % n), and {(dealer, round): oracle row} for the crafted dealers."""
    N = t + 1
    h = be.env_init(1, n, CK)
    a, b = crafted_coefficients(n, t, D, seed, rows, plen, sign, control)
    E, A, s, sp = (bytearray(x) for x in be.share_gen(a, b, D, n, t))
    exp = {}
    cut = lambda buf, w, i: bytes(buf[w * i:w * (i + 1)])  # noqa: E731
    for d in rows:
        oE, oA, os_, osp = O.share_gen(1, n, t, cut(a, 32 * N, d), cut(b, 32 * N, d), h)
        assert (cut(E, 32 * N, d), cut(A, 32 * N, d)) == (oE, oA), d  # the crafted commitments are the oracle's
        assert (cut(s, 32 * n, d), cut(sp, 32 * n, d)) == (os_, osp), d
        jb = (bump or {}).get(d, (d + 7) % n)
        _bump(s, 32 * (d * n + jb))
        # honest shares of a crafted (or control) row accept; exactly the bumped receiver rejects
        want = bytes(SELF if j == d else REJECT if j == jb else ACCEPT for j in range(n))
        for rnd, C in ((2, E), (4, A)):
            if oracle:
                acc, rc = O.verify_rows(n, t, rnd, cut(C, 32 * N, d), h, cut(s, 32 * n, d),
                                        cut(sp, 32 * n, d) if rnd == 2 else None, d, d + 1, 0, n)
                assert rc == 0 and acc == want, (d, rnd)
            exp[(d, rnd)] = want
    return E, A, s, sp, exp


def _run_case(be, n, t, D, U, rows, seed, modes=(0,), sign=+1, bump=None, redo=True, exact=None, ctl_oracle=True):
    """The common assertions (module docstring).  exact: {slot mode: redone workgroups per round}.
    ctl_oracle = False (the shapes whose oracle rows take seconds): the control rows are honest dealers
    with one bumped share, whose row holds by construction like every honest dealer's here -- commitments
    and shares of random polynomials from share_gen, asserted equal to the oracle's; g (s + 1) != g s."""
    plen = _plen(n, t, D, U)
    E, A, s, sp, exp = _committee(be, n, t, D, seed, rows, plen, sign, bump=bump)
    ref = _verify(be, n, t, D, E, A, s, sp, 1, formula=1)  # unsplit, complete additions
    assert ref[2:] == (0, 0)
    _check(n, D, ref[0], ref[1], exp, "unsplit complete")
    for mode in modes:
        d2, d4, r2, r4 = _verify(be, n, t, D, E, A, s, sp, U, stepping=mode)
        assert U == 1 or be.last_split_len() == plen
        print(f"n={n} t={t} U={U} D={D} mode={mode} sign={sign}: stepping redos {r2} / {r4}")
        _check(n, D, d2, d4, exp, (n, t, U, mode))
        assert (d2, d4) == ref[:2], mode
        if not redo:
            assert (r2, r4) == (0, 0), mode
        elif exact is not None:
            assert (r2, r4) == (exact[mode], exact[mode]), mode
        else:
            assert r2 > 0 and r4 > 0, mode
        c2, c4, q2, q4 = _verify(be, n, t, D, E, A, s, sp, U, stepping=mode, formula=1)
        assert (c2, c4) == (d2, d4) and (q2, q4) == (0, 0), mode
    # the control: every solved coefficient + 1, shares regenerated from it
    E, A, s, sp, exp = _committee(be, n, t, D, seed, rows, plen, sign, control=True, bump=bump, oracle=ctl_oracle)
    for mode in modes:
        d2, d4, r2, r4 = _verify(be, n, t, D, E, A, s, sp, U, stepping=mode)
        assert (r2, r4) == (0, 0), mode
        _check(n, D, d2, d4, exp, ("control", mode))


def _row(spec):
    seed, m, j = spec[:3]
    return dict(seed=seed, pairs=[(0, m, j)])


# ---- shape 1: t = 31, unsplit: the dead-position repack -------------------------------------------
# stepping_tail_phases(32, n, 1) = 4: phase k runs steps [J_k, J_(k+1)) on segments of P_k = 32 / 2^k
# lanes, J_k = n - P_k + 1 (0, 49, 57, 61 at n = 64; 0, 55, 63, 67 at n = 70).  Slot mode 3 runs the
# same table in one launch, without the repack.
# dkg_verify_pairs takes dealers [d0, d1) of the n parties (d1 <= n), so a ragged dealer group needs
# n = 70: 70 dealers are 64 + 6 columns, padded to 128.
# Redone workgroups: a crafted column meets its pair in ONE phase (the steps j above) and marks the
# one workgroup that holds it there; a workgroup of 32-lane segments holds 256 / 32 = 8 consecutive
# columns (stepping_shape), and the two crafted columns of phase 0 are more than 8 apart: 4 marked
# workgroups with the repack.  Without it the one launch's 8-column workgroups hold columns
# 0 | 21 | 37 | 63 (4 of them) at n = 64 and 0 | 63 | 64 and 69 (3) at n = 70.
def test_unsplit_tail_phases(be):
    rows = {d: _row(spec) for d, spec in SHAPE1.items()}
    _run_case(be, 64, 31, 64, 1, rows, seed=41, modes=(0, 3), exact={0: 4, 3: 4})


def test_unsplit_tail_phases_ragged_group_boundary(be):
    rows = {d: _row(spec) for d, spec in SHAPE1R.items()}
    _run_case(be, 70, 31, 70, 1, rows, seed=41, modes=(0, 3), exact={0: 4, 3: 3})


@pytest.mark.parametrize("spec", STEP_SEEDS, ids=lambda s: f"s{s[0]}m{s[1]}j{s[2]}{s[3]}{s[4]}")
def test_unsplit_one_pair_by_class(be, spec):
    """One crafted dealer per torsion class: one workgroup of one launch is redone in either slot mode."""
    _run_case(be, 64, 31, 64, 1, {37: _row(spec)}, seed=42, modes=(0, 3), exact={0: 1, 3: 1})


# ---- shape 2: n = 130, t = 127, 130 dealers, split ------------------------------------------------
# U, slot modes: U = 2 pieces of 64 (banded map, band 16, scaled state); U = 4 pieces of 32 as whole
# columns and per piece; U = 3 pieces 43 / 43 / 42 (contiguous map, k_affine_pieces<SC> with the dense
# Z copy).  Dealers 0, 65 and 129 sit in the first, a middle and the last stepping workgroup; their
# relations lie in piece 0, in the middle piece AND the one after it, and in the last (ragged) piece.
@pytest.mark.parametrize("U,modes", [(2, (0,)), (4, (1, 2)), (3, (0,))])
def test_split_pieces(be, U, modes):
    n, t, D = 130, 127, 130
    plen = _plen(n, t, D, U)
    last = t + 1 - (U - 1) * plen
    assert (plen, last) == {2: (64, 64), 4: (32, 32), 3: (43, 42)}[U]
    mid = U // 2
    rows = {0: dict(seed=11, pairs=[(0, 5, 40)]),
            65: dict(seed=12, pairs=[(mid, 2, 90), ((mid + 1) % U, 20, 3)]),
            129: dict(seed=13, pairs=[(U - 1, min(last - 2, 17), 100)])}
    # U = 4 with the slot mode forced: one slot per column (mode 1) puts all pieces of a column into one
    # workgroup, and the three crafted columns are further apart than any workgroup is wide: 3; one
    # launch row per piece (mode 2) has a workgroup per (columns, piece), and the four (dealer, piece)
    # relations are pairwise apart in column or piece: 4.  Mode 0's layout is the cost model's choice.
    _run_case(be, n, t, D, U, rows, seed=43, modes=modes, exact={1: 3, 2: 4} if U == 4 else None)


# ---- shape 3: pieces of 515 positions in two 258-position blocks ----------------------------------
def test_multiblock_pieces_across_the_stream(be):
    """n = 1040, t = 1029, U = 2 (the shape of test_scaled_streams_of_multiblock_pieces).  Dealer 1's
    pair is at position 257, the lower block's top lane, whose addend is the value streamed down from
    the block above; dealer 2's at position 258, the upper block's position 0, which feeds that
    stream; both at step 300, long after the stream started.  One workgroup per (column, piece) and
    one flag word for a column's blocks: dealer 1 marks piece 1, dealer 2 piece 0 -- 2 words."""
    n, t, D = 1040, 1029, 4
    rows = {1: dict(seed=21, pairs=[(1, 257, 300)]), 2: dict(seed=22, pairs=[(0, 258, 300)])}
    _run_case(be, n, t, D, 2, rows, seed=44, exact={0: 2}, ctl_oracle=False)


# ---- shape 4: unsplit two-block tables with proper streams ----------------------------------------
def test_unsplit_multiblock_across_the_stream(be):
    """n = 610, t = 599, unsplit: stepping_shape(600) is two blocks of 300 positions (320-lane
    workgroups, one column each, proper cached forms in the stream).  Dealer 0's pair is at position
    299 (the lower block's top lane), dealer 2's at position 300 (the upper block's position 0), both
    at step 300; dealer 1 is honest.  One flag word per column: 2."""
    n, t, D = 610, 599, 3
    rows = {0: dict(seed=31, pairs=[(0, 299, 300)]), 2: dict(seed=32, pairs=[(0, 300, 300)])}
    _run_case(be, n, t, D, 1, rows, seed=45, exact={0: 2}, ctl_oracle=False)


# ---- shape 5: opposite pairs ---------------------------------------------------------------------
@pytest.mark.parametrize("spec", OPP_SEEDS, ids=lambda s: f"s{s[0]}{s[3]}{s[4]}")
def test_opposite_pairs_unsplit(be, spec):
    """Q(20) = -Delta Q(20): the dedicated addition is not exceptional there (F, G != 0, as the CPU
    model asserts for these seeds), its sum Q(21) is a pure torsion point -- O, T2 or an order-4 point
    with Y = 0 -- and both shares of receiver 20 are zero.  Nothing is redone, every check accepts
    (the checks' second equality branch for T4), and the bumped zero share rejects."""
    seed, m, j = spec[:3]
    _run_case(be, 64, 31, 64, 1, {37: _row(spec)}, seed=46, modes=(0, 3), sign=-1, bump={37: j}, redo=False)


def test_opposite_pairs_split(be):
    """n = 130 at U = 2 with the opposite pair in BOTH pieces at step 20, so that P(21) is the identity
    class and both shares of receiver 20 are zero: the affine normalisation takes two pure torsion
    values (k_affine_pairs)."""
    rows = {65: dict(seed=14, pairs=[(0, 0, 20), (1, 0, 20)])}
    _run_case(be, 130, 127, 130, 2, rows, seed=47, sign=-1, bump={65: 20}, redo=False)


# ---- shapes 6 and 7: the binomial, n = 64, t = 31, whole ceremonies --------------------------------
KEYS = ("dec2", "dec4", "qualified", "reconstruct", "final_share", "public_share", "mpk")


def _ceremony_inputs(be, rows, plen, sign=+1, control=False, seed=48, bump=(5, 9)):
    """A whole n = 64 committee's broadcasts with the dealers of `rows` crafted; those also in `bump`
    get one wrong share (a complaint disqualifies them: their round-4 row is skipped), the others stay
    qualified, so their commitments reach the final shares, the public shares and the mpk."""
    n, t = 64, 31
    N = t + 1
    h = be.env_init(t, n, CK)
    a, b = crafted_coefficients(n, t, n, seed, rows, plen, sign, control)
    E, A, s, sp = (bytearray(x) for x in be.share_gen(a, b, n, n, t))
    exp = {}
    cut = lambda buf, w, i: bytes(buf[w * i:w * (i + 1)])  # noqa: E731
    for d in rows:
        oE, oA, _, _ = O.share_gen(1, n, t, cut(a, 32 * N, d), cut(b, 32 * N, d), h)
        assert (cut(E, 32 * N, d), cut(A, 32 * N, d)) == (oE, oA), d
        if d in bump:
            _bump(s, 32 * (d * n + (d + 7) % n))
        for rnd, C in ((2, E), (4, A)):
            acc, rc = O.verify_rows(n, t, rnd, cut(C, 32 * N, d), h, cut(s, 32 * n, d),
                                    cut(sp, 32 * n, d) if rnd == 2 else None, d, d + 1, 0, n)
            assert rc == 0
            exp[(d, rnd)] = acc
    return bytes(E), bytes(A), bytes(s), bytes(sp), exp


def _outs(r):
    return tuple(bytes(getattr(r, k)) if isinstance(getattr(r, k), (bytes, bytearray)) else getattr(r, k)
                 for k in KEYS)


def _check_rows(r, exp, n=64):
    for (d, rnd), want in exp.items():
        dec = bytes(r.dec2 if rnd == 2 else r.dec4)
        # a ceremony's round 4 runs after round 2's outcomes: compare the pairs the oracle decides
        got = dec[d * n:(d + 1) * n]
        if rnd == 2:
            assert got == want, (d, rnd)
        else:
            assert all(g == w for g, w in zip(got, want) if g in (ACCEPT, REJECT, SELF)), (d, rnd)


@pytest.mark.parametrize("spec", BINOM_SEEDS, ids=lambda s: f"s{s[0]}r{s[1]}m{s[2]}{'p' if s[3] > 0 else 'n'}")
def test_per_step_binomial_pair(be, spec):
    """The step-r input of dealers 5 (one wrong share) and 41 (qualified) has e_(m-1) = +-e_m.  Without
    lane pairs (dkg_ctx_set_binomial 1) the
    step's dedicated item marks the guard word and the driver reruns the verification -- exactly
    when the CPU model of the item (addition, then the m-chain) meets Z = 0; the outputs equal the
    complete formula's and the default schedule's either way, and the control reruns nothing."""
    seed, r, m, sign, _, _, rerun = spec
    n, t = 64, 31
    rows = {5: dict(seed=seed, binom=[(0, r, m)]), 41: dict(seed=seed + 100, binom=[(0, r, m)])}
    E, A, s, sp, exp = _ceremony_inputs(be, rows, t + 1, sign)
    try:
        be.set_binomial(1)
        r1 = be.ceremony_verify(E, A, s, sp, n, t)
        assert be.binomial_reruns() == (1 if rerun else 0)
        assert be.last_binomial() == 0
        be.set_stepping_formula(1)
        rc = be.ceremony_verify(E, A, s, sp, n, t)
        assert be.binomial_reruns() == 0
        be.set_stepping_formula(0)
        be.set_binomial(0)
        r0 = be.ceremony_verify(E, A, s, sp, n, t)
        _check_rows(r1, exp)
        assert _outs(r1) == _outs(rc) and _outs(r0) == _outs(rc)
        Ec, Ac, sc, spc, expc = _ceremony_inputs(be, rows, t + 1, sign, control=True)
        be.set_binomial(1)
        r2 = be.ceremony_verify(Ec, Ac, sc, spc, n, t)
        assert be.binomial_reruns() == 0 and be.stepping_redos() == 0
        _check_rows(r2, expc)
    finally:
        be.set_stepping_formula(0)
        be.set_binomial(0)


@pytest.mark.parametrize("spec", WAVE_SEEDS, ids=lambda s: f"s{s[0]}r{s[2]}m{s[3]}")
def test_per_wave_binomial_pair(be, spec):
    """dkg_ctx_set_binomial 4 with a 2-way split forced (pieces of 16): dealers 5 and 41 carry the pair
    in piece 1, in the sharing and the hiding polynomial alike.  The fused pipeline lays a dealer group
    out as 64 E columns then 64 A columns (npad = 128), one flag word per (piece, 64 columns): both
    dealers mark word piece 1 x E and word piece 1 x A and nothing else -- 2 words."""
    seed, piece, r, m = spec
    n, t = 64, 31
    rows = {5: dict(seed=seed, binom=[(piece, r, m)]), 41: dict(seed=seed + 100, binom=[(piece, r, m)])}
    E, A, s, sp, exp = _ceremony_inputs(be, rows, 16)
    try:
        be.set_binomial(4)
        be.set_split(2)
        r4 = be.ceremony_verify(E, A, s, sp, n, t)
        assert be.last_binomial() == 1 and be.last_split() == 2 and be.last_split_len() == 16
        assert be.binomial_wave_redos() == 2
        assert be.binomial_reruns() == 0
        _check_rows(r4, exp)
        be.set_stepping_formula(1)
        rc = be.ceremony_verify(E, A, s, sp, n, t)
        assert be.binomial_wave_redos() == 0
        be.set_stepping_formula(0)
        be.set_binomial(1)
        r1 = be.ceremony_verify(E, A, s, sp, n, t)
        assert be.binomial_wave_redos() == 0  # the per-step schedule marks no (piece, group) word
        assert _outs(r4) == _outs(rc) and _outs(r4) == _outs(r1)
        Ec, Ac, sc, spc, expc = _ceremony_inputs(be, rows, 16, control=True)
        be.set_binomial(4)
        r2 = be.ceremony_verify(Ec, Ac, sc, spc, n, t)
        assert be.binomial_wave_redos() == 0 and be.stepping_redos() == 0
        _check_rows(r2, expc)
    finally:
        be.set_stepping_formula(0)
        be.set_binomial(0)
        be.set_split(0)


def test_per_wave_binomial_batch(be):
    """Three ceremonies in one batch under the per-wave binomial, unsplit (tail phases): dealers 9 and 41
    of ceremony 1 have a binomial pair at (20, 7) and a stepping pair at (1, 58), a late tail phase.  Every
    per-ceremony output equals the three single calls and the complete-formula batch; both counters are
    > 0, and 0 for the control batch."""
    n, t = 64, 31
    rows = {9: BATCH_ROW, 41: dict(BATCH_ROW, seed=BATCH_ROW["seed"] + 100)}  # 9 with a wrong share, 41 qualified
    honest = _ceremony_inputs(be, {}, t + 1, seed=49)[:4]
    other = _ceremony_inputs(be, {}, t + 1, seed=50)[:4]
    E, A, s, sp, exp = _ceremony_inputs(be, rows, t + 1, seed=51)
    cat = lambda k: honest[k] + (E, A, s, sp)[k] + other[k]  # noqa: E731
    try:
        be.set_binomial(4)
        rb = dkg_amd.ceremony_batch_verify(be, 3, n, t, cat(0), cat(1), cat(2), cat(3))
        wave, step = be.binomial_wave_redos(), be.stepping_redos()
        print(f"batch: wave redos {wave}, stepping redos {step}")
        assert wave > 0 and step > 0
        singles = []
        for c, x in enumerate((honest, (E, A, s, sp), other)):
            singles.append(be.ceremony_verify(*x, n, t))
            wave, step = be.binomial_wave_redos(), be.stepping_redos()
            assert (wave > 0 and step > 0) if c == 1 else (wave, step) == (0, 0), c
        _check_rows(singles[1], exp)
        be.set_stepping_formula(1)
        rc = dkg_amd.ceremony_batch_verify(be, 3, n, t, cat(0), cat(1), cat(2), cat(3))
        assert be.binomial_wave_redos() == 0 and be.stepping_redos() == 0
        be.set_stepping_formula(0)
        for c in range(3):
            got, want = rb.ceremony(c), rc.ceremony(c)
            for k in KEYS:
                assert got[k] == want[k], (c, k)
                one = getattr(singles[c], k)
                assert (bytes(got[k]) if isinstance(one, (bytes, bytearray)) else list(got[k])) == \
                       (bytes(one) if isinstance(one, (bytes, bytearray)) else list(one)), (c, k)
        Ec, Ac, sc, spc, _ = _ceremony_inputs(be, rows, t + 1, control=True, seed=51)
        ctl = lambda k: honest[k] + (Ec, Ac, sc, spc)[k] + other[k]  # noqa: E731
        dkg_amd.ceremony_batch_verify(be, 3, n, t, ctl(0), ctl(1), ctl(2), ctl(3))
        assert be.binomial_wave_redos() == 0 and be.stepping_redos() == 0
    finally:
        be.set_stepping_formula(0)
        be.set_binomial(0)
