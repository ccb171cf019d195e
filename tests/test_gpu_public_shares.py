"""dkg_commitment_sum and dkg_public_shares (pubshares.hip k_commit_colsum, the receivers' evaluator on the
summed table) against the libsodium fixtures, tests/public_share_ref.py and whole ceremonies, byte for byte."""
import ctypes
import random

import pytest

import dkg_amd
from dkg_amd import DKG_PS_NO_COMMITMENT, DKG_PS_NO_DISCLOSURE, DKG_PS_OK, DkgError
from tests import public_share_ref as PR
from tests import ristretto_ref as R

pytestmark = pytest.mark.gpu

H = bytes.fromhex
CK = b"Example of a shared string."
ZERO = bytes(32)
FIXTURES = ["ceremony_n10_t4", "fault_recon_only_n10_t4", "fault_share_flip_n10_t4", "fault_a_generator_n10_t4",
            "fault_self_share_n10_t4", "fault_e_identity_n10_t4", "fault_recon_r2err_n16_t3", "ceremony_n2_t0",
            "ceremony_n3_t1", "ceremony_n11_t5", "ceremony_n16_t7", "ceremony_n8_t3_ck", "ceremony_n64_t31"]
STACK = FIXTURES[:6]  # the n = 10, t = 4 fixtures


@pytest.fixture(scope="module")
def be():
    b = dkg_amd.Backend(0)
    yield b
    b.close()


def stacked(golden, names):
    """(A, qualified, reconstruct, disclosures) of the fixtures `names` as the ceremonies of one batch."""
    A, q, r, dis = b"", [], [], []
    for g, name in enumerate(names):
        c = golden(name + ".json")
        A += H(c["A"])
        q += c["qualified"]
        r += c["reconstruct"]
        dis += PR.fixture_disclosures(c, g)
    return A, q, r, dis


# ---------------------------------------------------------------- 1. single-ceremony fixtures
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture(be, golden, name):
    c = golden(name + ".json")
    n, t = c["n"], c["t"]
    A, q, r = H(c["A"]), c["qualified"], c["reconstruct"]
    dis = PR.fixture_disclosures(c)
    out = be.public_shares(1, n, t, A, q, list(range(n)), r, dis, want_sum=True)
    assert out.status == [DKG_PS_OK] * n and out.which == [-1] * n
    assert out.V == H(c["public_share"])
    mask = [int(a and not b) for a, b in zip(q, r)]
    S, ok = PR.commitment_sum(1, n, t, A, mask)
    assert ok == [1] and out.S == S
    assert be.commitment_sum(1, n, t, A, mask) == (S, b"\x01")
    if not any(r):
        assert out.S[:32] == H(c["mpk"])
        assert be.public_shares(1, n, t, A, q, list(range(n))).V == out.V  # reconstruct NULL, no S


# ---------------------------------------------------------------- 2. a missing disclosure
def test_missing_disclosure(be, golden):
    c = golden("fault_recon_only_n10_t4.json")
    n, t = c["n"], c["t"]
    A, q, r = H(c["A"]), c["qualified"], c["reconstruct"]
    dis = PR.fixture_disclosures(c)
    js = list(range(n))
    full = be.public_shares(1, n, t, A, q, js, r, dis, want_sum=True)
    rec = [i for i in range(n) if r[i]]
    drop = (0, 6, rec[1] + 1)  # party 5 (0-based) keeps its share of the second reconstructed dealer
    less = [d for d in dis if d[:3] != drop]
    assert len(less) == len(dis) - 1
    out = be.public_shares(1, n, t, A, q, js, r, less, want_sum=True)
    assert out.status == [DKG_PS_NO_DISCLOSURE if j == 5 else DKG_PS_OK for j in js]
    assert out.which == [rec[1] if j == 5 else -1 for j in js]
    assert out.S == full.S
    for j in js:
        assert out.V[32 * j:32 * j + 32] == (ZERO if j == 5 else full.V[32 * j:32 * j + 32])
    # the flat form of the disclosures, and an entry of a sender outside js
    flat = ([d[0] for d in less], [d[1] for d in less], [d[2] for d in less], b"".join(d[3] for d in less))
    sub = be.public_shares(1, n, t, A, q, [4, 2], r, flat)
    assert sub.status == [DKG_PS_OK] * 2
    assert sub.V == full.V[32 * 4:32 * 5] + full.V[32 * 2:32 * 3]


# ---------------------------------------------------------------- 3. batches
def test_batches(be, golden):
    n, t = 10, 4
    js = [7, 0, 3, 3, 9, 1, 8, 2, 6, 5, 4]  # unordered, one repeat
    M = len(js)
    single = []
    for name in STACK:
        c = golden(name + ".json")
        o = be.public_shares(1, n, t, H(c["A"]), c["qualified"], js, c["reconstruct"], PR.fixture_disclosures(c),
                             want_sum=True)
        assert o.status == [DKG_PS_OK] * M
        assert o.V == b"".join(H(c["public_share"])[32 * j:32 * j + 32] for j in js)
        single.append(o)
    A, q, r, dis = stacked(golden, STACK)
    out = be.public_shares(len(STACK), n, t, A, q, js, r, dis, want_sum=True)
    assert out.V == b"".join(o.V for o in single) and out.S == b"".join(o.S for o in single)
    assert out.status == [DKG_PS_OK] * (len(STACK) * M)
    # B = 130: more than two wave columns of rows in the evaluator, the last one partial
    names = (STACK * 22)[:130]
    A, q, r, dis = stacked(golden, names)
    random.Random(5).shuffle(dis)
    out = be.public_shares(130, n, t, A, q, js, r, dis, want_sum=True)
    assert out.status == [DKG_PS_OK] * (130 * M) and out.which == [-1] * (130 * M)
    assert out.V == b"".join(single[g % len(STACK)].V for g in range(130))
    assert out.S == b"".join(single[g % len(STACK)].S for g in range(130))


# ---------------------------------------------------------------- 4. dealer tiles
@pytest.mark.parametrize("n", [130, 128])
def test_dealer_tiles(be, n):
    t = 3
    be.env_init(t, n, CK)
    a, b = dkg_amd.dealer_coefficients(bytes([n]) * 32, 1, 0, n, t)
    A = be.share_gen(a, b, n, n, t)[1]
    rng = random.Random(n)
    mask = [int(rng.random() < 0.7) for _ in range(n)]
    mask[n - 1] = 1
    S, ok = PR.commitment_sum(1, n, t, A, mask)
    assert be.commitment_sum(1, n, t, A, mask) == (S, b"\x01")
    js = [0, n - 1, 64]
    V, st, wh, S2 = PR.public_shares(1, n, t, A, mask, js)
    out = be.public_shares(1, n, t, A, mask, js, want_sum=True)
    assert (out.V, out.status, out.which, out.S) == (V, st, wh, S) and S2 == S
    assert be.commitment_sum(1, n, t, A) == (PR.commitment_sum(1, n, t, A)[0], b"\x01")  # NULL mask: all dealers


# ---------------------------------------------------------------- 5. identity sums
def test_identity_sums(be, golden):
    c = golden("ceremony_n3_t1.json")
    t = 1
    row = H(c["A"])[:64]
    A = row + b"".join(R.encode(R.neg(R.decode(row[32 * k:32 * k + 32]))) for k in range(2))  # A_2 = -A_1
    out = be.public_shares(1, 2, t, A, [1, 1], [0, 1], want_sum=True)
    assert out.S == ZERO * 2 and out.V == ZERO * 2 and out.status == [DKG_PS_OK] * 2
    assert be.commitment_sum(1, 2, t, A) == (ZERO * 2, b"\x01")
    assert be.commitment_sum(1, 2, t, A, [1, 0]) == (row, b"\x01")
    # an all-zero mask: the identity in every coefficient
    out = be.public_shares(1, 2, t, A, [0, 0], [1, 0, 1], want_sum=True)
    assert out.S == ZERO * 2 and out.V == ZERO * 3 and out.status == [DKG_PS_OK] * 3
    assert be.commitment_sum(1, 2, t, A, [0, 0]) == (ZERO * 2, b"\x01")


# ---------------------------------------------------------------- 6. undecodable and absent rows
def test_undecodable_rows(be, golden):
    c = golden("ceremony_n10_t4.json")
    n, t, N = c["n"], c["t"], c["t"] + 1
    A1 = H(c["A"])
    js = [2, 9, 0]
    good = be.public_shares(1, n, t, A1, c["qualified"], js, want_sum=True)
    bad = bytearray(A1 * 3)
    k = 32 * ((n + 4) * N + 2)  # ceremony 1, dealer 4, coefficient 2
    bad[k:k + 32] = b"\xff" * 32
    bad = bytes(bad)
    q = [1] * (3 * n)
    out = be.public_shares(3, n, t, bad, q, js, want_sum=True)
    assert out.status == [DKG_PS_OK] * 3 + [DKG_PS_NO_COMMITMENT] * 3 + [DKG_PS_OK] * 3
    assert out.which == [-1] * 3 + [4] * 3 + [-1] * 3
    assert out.V == good.V + ZERO * 3 + good.V
    assert out.S == good.S + ZERO * N + good.S
    assert be.commitment_sum(3, n, t, bad) == (out.S, b"\x01\x00\x01")
    # the same row masked out is never interpreted
    q[n + 4] = 0
    out = be.public_shares(3, n, t, bad, q, js, want_sum=True)
    assert out.status == [DKG_PS_OK] * 9 and out.which == [-1] * 9
    V, st, wh, S = PR.public_shares(3, n, t, bad, q, js)
    assert (out.V, out.S) == (V, S)
    assert be.commitment_sum(3, n, t, bad, q) == (S, b"\x01\x01\x01")
    # fetched3 = 0 on a used dealer behaves like the undecodable row; on an unused one it changes nothing
    f3 = [1] * (3 * n)
    f3[2 * n + 7] = f3[2 * n + 3] = f3[n + 4] = 0
    out = be.public_shares(3, n, t, bad, q, js, fetched3=f3, want_sum=True)
    assert out.status == [DKG_PS_OK] * 6 + [DKG_PS_NO_COMMITMENT] * 3
    assert out.which == [-1] * 6 + [3] * 3
    assert out.V == V[:32 * 6] + ZERO * 3 and out.S == S[:32 * N * 2] + ZERO * N


# ---------------------------------------------------------------- 7. option independence
def test_options(be, golden):
    n, t = 10, 4
    names = (STACK * 2)[:7]
    A, q, r, dis = stacked(golden, names)
    js = list(range(n))

    def run():
        o = be.public_shares(len(names), n, t, A, q, js, r, dis, want_sum=True)
        return o.V, o.status, o.which, o.S, be.commitment_sum(len(names), n, t, A, q)

    base = run()
    assert base[0] == b"".join(H(golden(x + ".json")["public_share"]) for x in names)
    try:
        for slab in (3, 1, 10, 64):  # 3 cuts through ceremonies
            be.set_public_share_slab(slab)
            assert run() == base, slab
        be.set_public_share_slab(0)
        for mode in (1, 2):
            be.set_field_mode(mode)
            assert run() == base, mode
        be.set_field_mode(0)
        for chunk in (1, 2, t + 1):
            be.set_receiver_chunk(chunk)
            assert run() == base, chunk
            assert be.last_receiver_chunk() == chunk
    finally:
        be.set_public_share_slab(0)
        be.set_field_mode(0)
        be.set_receiver_chunk(0)
    assert run() == base


# ---------------------------------------------------------------- 8. a whole ceremony at (256, 127)
def test_whole_ceremony(be):
    n, t = 256, 127
    be.env_init(t, n, CK)
    a, b = dkg_amd.dealer_coefficients(b"\x42" * 32, 3, 0, n, t)
    r = be.ceremony(a, b, n, t)
    assert not any(r.reconstruct) and all(r.qualified)
    out = be.public_shares(1, n, t, r.A, r.qualified, list(range(n)), r.reconstruct, want_sum=True)
    assert out.status == [DKG_PS_OK] * n
    assert out.V == r.public_share
    assert out.S[:32] == r.mpk


# ---------------------------------------------------------------- 9. argument rules
def test_arguments(be, golden):
    c = golden("fault_recon_only_n10_t4.json")
    n, t = c["n"], c["t"]
    A, q, r = H(c["A"]), c["qualified"], c["reconstruct"]
    dis = PR.fixture_disclosures(c)
    for kw in [dict(js=[0, n]),                                                  # js[m] >= n
               dict(q=[0 if r[i] else 1 for i in range(n)]),                     # reconstruct without qualified
               dict(dis=dis + [dis[3]]),                                         # a duplicate disclosure
               dict(dis=dis + [(1, 1, 1, ZERO)]),                                # ceremony out of range
               dict(dis=dis + [(0, n + 1, 1, ZERO)]), dict(dis=dis + [(0, 1, 0, ZERO)])]:
        with pytest.raises(DkgError) as e:
            be.public_shares(1, n, t, A, kw.get("q", q), kw.get("js", [0, 1]), r, kw.get("dis", dis))
        assert e.value.code == -1
    L = dkg_amd.lib()
    u8 = lambda v: bytes(bytearray(v))  # noqa: E731
    one = (ctypes.c_uint32 * 1)(0)
    V = ctypes.create_string_buffer(b"\x07" * 32, 32)
    st = (ctypes.c_int32 * 1)(7)
    # a NULL required pointer
    assert L.dkg_public_shares(be.ctx, 1, n, t, None, u8(q), None, None, 1, one, 0, None, None, None, None, V, st, None, None) == -1
    assert L.dkg_public_shares(be.ctx, 1, n, t, A, None, None, None, 1, one, 0, None, None, None, None, V, st, None, None) == -1
    assert L.dkg_public_shares(be.ctx, 1, n, t, A, u8(q), None, None, 1, None, 0, None, None, None, None, V, st, None, None) == -1
    assert L.dkg_public_shares(be.ctx, 1, n, t, A, u8(q), None, None, 1, one, 0, None, None, None, None, None, st, None, None) == -1
    assert L.dkg_public_shares(be.ctx, 1, n, t, A, u8(q), None, None, 1, one, 0, None, None, None, None, V, None, None, None) == -1
    assert L.dkg_public_shares(be.ctx, 1, n, t, A, u8(q), None, None, 1, one, 1, one, one, None, None, V, st, None, None) == -1
    assert L.dkg_commitment_sum(be.ctx, 1, n, t, None, None, V, None) == -1
    assert L.dkg_commitment_sum(be.ctx, 1, n, t, A, None, None, None) == -1
    # B == 0 or M == 0 touches nothing
    assert L.dkg_public_shares(be.ctx, 0, n, t, None, None, None, None, 1, one, 0, None, None, None, None, V, st, None, None) == 0
    assert L.dkg_public_shares(be.ctx, 1, n, t, A, u8(q), None, None, 0, None, 0, None, None, None, None, V, st, None, None) == 0
    assert L.dkg_commitment_sum(be.ctx, 0, n, t, None, None, V, None) == 0
    assert V.raw == b"\x07" * 32 and st[0] == 7
    assert be.public_shares(1, n, t, A, q, [], r, dis).V == b""
    with pytest.raises(DkgError):
        be.set_public_share_slab(2**30 + 1)


# ---------------------------------------------------------------- 10. phase records
def test_phase_records(golden):
    c = golden("fault_recon_only_n10_t4.json")
    n, t = c["n"], c["t"]
    A, q, r = H(c["A"]), c["qualified"], c["reconstruct"]
    h = golden("ceremony_n10_t4.json")
    b = dkg_amd.Backend(0)
    try:
        b.set_streams(1)
        b.public_shares(1, n, t, A, q, list(range(n)), r, PR.fixture_disclosures(c))
        ph = b.phase_times("pubshares")
        assert all(ph[k] >= 0 for k in ("decode", "sum", "eval", "disclosed")), ph
        b.public_shares(1, n, t, H(h["A"]), h["qualified"], list(range(n)))
        ph = b.phase_times("pubshares")
        assert all(ph[k] >= 0 for k in ("decode", "sum", "eval")) and ph["disclosed"] == -1, ph
        b.commitment_sum(1, n, t, A)
        ph = b.phase_times("pubshares")
        assert ph["decode"] >= 0 and ph["sum"] >= 0 and ph["eval"] == -1 and ph["disclosed"] == -1, ph
    finally:
        b.close()
