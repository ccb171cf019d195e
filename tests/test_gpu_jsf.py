"""The pairwise joint-sparse-form recombination (k_pair_sums, k_combine_jsf: the default at U = 2 and
4) against today's per-scalar NAF chains (dkg_ctx_set_combine 3), the golden fixtures and the CPU
oracle.  Bit-exact throughout: decisions, qualified sets and the master public key do not depend on
the recombination."""
import pytest

import dkg_amd
from dkg_amd import ACCEPT, REJECT, SELF
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

H = bytes.fromhex
ELL = 2**252 + 27742317777372353535851937790883648493
CK = b"Example of a shared string."
FAULTS = ["fault_e_identity_n10_t4.json", "fault_share_flip_n10_t4.json",
          "fault_a_generator_n10_t4.json", "fault_over_threshold_n10_t4.json", "fault_a_many_n10_t4.json",
          "fault_self_share_n10_t4.json", "fault_recon_only_n10_t4.json", "fault_recon_r2err_n16_t3.json",
          "fault_recon_insufficient_n16_t3.json"]


@pytest.fixture(scope="module")
def be():
    b = dkg_amd.Backend(0)
    yield b
    b.close()


def dec_str(raw):
    return "".join(str(x) for x in raw)


def _outputs(r):
    return (bytes(r.dec2), bytes(r.dec4), r.qualified, r.reconstruct, r.complaints2, r.final_share, r.public_share,
            r.mpk)


def _both_modes(be, pieces, run):
    """run() under the default recombination and under mode 3 with a forced split; both results."""
    out = []
    try:
        be.set_split(pieces)
        for mode in (0, 3):
            be.set_combine(mode)
            out.append(run())
            assert be.last_split() == pieces and be.last_combine() == 2
    finally:
        be.set_combine(0)
        be.set_split(0)
    return out


# n = 64 with pieces of 16 and 8 positions; the n = 10 fault fixtures and n = 11 (receiver counts
# that fill neither a wave of columns nor a run of the normalisation; t + 1 = 5 and 6 positions)
@pytest.mark.parametrize("pieces", [2, 4])
@pytest.mark.parametrize("name", ["ceremony_n64_t31.json", "ceremony_n11_t5.json"] + FAULTS)
def test_jsf_matches_naf_and_goldens(be, golden, name, pieces):
    c = golden(name)
    n, t = c["n"], c["t"]
    be.env_init(t, n, CK)
    r0, r3 = _both_modes(be, pieces, lambda: be.ceremony_verify(H(c["E"]), H(c["A"]), H(c["s"]), H(c["s_prime"]), n, t))
    assert _outputs(r0) == _outputs(r3)
    for r in (r0, r3):
        assert dec_str(r.dec2) == c["dec2"] and dec_str(r.dec4) == c["dec4"]
        assert r.qualified == c["qualified"] and r.reconstruct == c["reconstruct"]
        assert r.mpk.hex() == c["mpk"] and r.final_share.hex() == c["final_share"]


@pytest.mark.parametrize("pieces", [2, 4])
def test_jsf_crafted_pairs_n64(be, pieces):
    """Dealers whose pieces 0 and 1 are equal (Q_0(j) - Q_1(j) is the identity at every receiver) and
    opposite (the sum is), honestly shared, so that every check accepts through the exceptional pair
    sums; the same in the last pair of pieces; and an all-identity E row.  Both chains give the
    oracle's rows."""
    n, t = 64, 31
    N, Lp = t + 1, (t + 1) // pieces
    h = be.env_init(t, n, CK)
    a, b = (bytearray(x) for x in dkg_amd.dealer_coefficients(bytes(range(32)), 21, 0, n, t))

    def tie(buf, dealer, dst, src, sign):
        for k in range(Lp):
            v = int.from_bytes(buf[32 * (dealer * N + src * Lp + k):32 * (dealer * N + src * Lp + k) + 32], "little")
            buf[32 * (dealer * N + dst * Lp + k):32 * (dealer * N + dst * Lp + k) + 32] = \
                (sign * v % ELL).to_bytes(32, "little")

    for buf in (a, b):
        tie(buf, 5, 1, 0, 1)              # dealer 5: piece 1 = piece 0
        tie(buf, 6, 1, 0, -1)             # dealer 6: piece 1 = -piece 0
        tie(buf, 8, pieces - 1, pieces - 2, 1)    # dealers 8, 9: the same in the last pair
        tie(buf, 9, pieces - 1, pieces - 2, -1)
    E, A, s, sp = (bytearray(x) for x in be.share_gen(bytes(a), bytes(b), n, n, t))
    assert E[32 * (5 * N + Lp):32 * (5 * N + 2 * Lp)] == E[32 * 5 * N:32 * (5 * N + Lp)]
    E[32 * 7 * N:32 * 8 * N] = bytes(32 * N)      # dealer 7: an all-identity E row
    r0, r3 = _both_modes(be, pieces, lambda: be.ceremony_verify(bytes(E), bytes(A), bytes(s), bytes(sp), n, t))
    assert _outputs(r0) == _outputs(r3)
    for i in (5, 6, 7, 8, 9):
        for rnd, C, dec in ((2, E, r0.dec2), (4, A, r0.dec4)):
            acc, _ = O.verify_rows(n, t, rnd, bytes(C[32 * N * i:32 * N * (i + 1)]), h, bytes(s[32 * n * i:32 * n * (i + 1)]),
                                   bytes(sp[32 * n * i:32 * n * (i + 1)]) if rnd == 2 else None, i, i + 1, 0, n)
            exp = bytes(SELF if j == i else (REJECT if (i, rnd) == (7, 2) else ACCEPT) for j in range(n))
            assert bytes(acc) == exp, ("the oracle on the crafted row", i, rnd)
            if (i, rnd) != (7, 4):   # dealer 7 is disqualified in round 2: its round-4 row is skipped
                assert bytes(dec[i * n:(i + 1) * n]) == exp, (i, rnd)
    assert r0.qualified == [int(i != 7) for i in range(n)]
    honest = bytes(SELF if j == 0 else ACCEPT for j in range(n))
    assert bytes(r0.dec2[:n]) == honest and bytes(r0.dec4[:n]) == honest


def test_jsf_sharded_verify_n64(be, golden):
    """The dealer-shard entry point (dkg_ceremony_shard_verify_device, three ranks played in one
    process; pieces of 8): the default chain and mode 3 give the golden ceremony."""
    import torch

    from tests import shard_play

    c = golden("ceremony_n64_t31.json")
    n, t = c["n"], c["t"]
    N = t + 1
    be.env_init(t, n, CK)
    dev = torch.device("cuda", 0)
    E, A, s, sp = (H(c[k]) for k in ("E", "A", "s", "s_prime"))
    keep = []

    def put(x):
        v = torch.frombuffer(bytearray(x or b"\0"), dtype=torch.uint8).to(dev)
        keep.append(v)
        return v

    def call(r, d0, d1, o2, o4, oA, op):
        tE, tA = put(E[32 * N * d0:32 * N * d1]), put(A[32 * N * d0:32 * N * d1])
        ts, tsp = put(s[32 * n * d0:32 * n * d1]), put(sp[32 * n * d0:32 * n * d1])
        be.ceremony_shard_verify_device(n, t, d0, d1, tE.data_ptr(), tA.data_ptr(), ts.data_ptr(), tsp.data_ptr(),
                                        o2.data_ptr(), o4.data_ptr(), oA.data_ptr(), op.data_ptr())
        return ts

    p0, p3 = _both_modes(be, 4, lambda: shard_play.play(be, n, t, 3, call, dev))
    for p in (p0, p3):
        assert dec_str(p.dec2) == c["dec2"] and dec_str(p.dec4) == c["dec4"]
        assert p.outcome.qualified == c["qualified"] and p.mpk.hex() == c["mpk"]
    assert (p0.dec2, p0.raw4, p0.final_share, p0.public_share) == (p3.dec2, p3.raw4, p3.final_share, p3.public_share)
