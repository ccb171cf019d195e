"""Full (encrypted-share) mode of the dealer-sharded ceremony: dkg_ceremony_shard_full_device /
_shard_verify_full_device per shard, dkg_multi_ceremony_run_full / _run_full_device / _verify_full over the
shards of one process, and the two combs of the recipient keys behind K = pk_q r (dkg_ctx_set_key_comb:
1 radix 2^10 tables, 2 signed radix-16 combs with D != n dealers per key, 0 the cost rule).  On a one-GPU
box the devices repeat ([0, 0], [0, 0, 0]).  Every output is compared byte for byte with the libsodium
fixtures, the CPU oracle or the single-context full-mode run."""
import ctypes
import hashlib
import random

import pytest

import dkg_amd
from dkg_amd import MISSING, SELF, _lib
from tests import edge_vectors as EV
from tests import oracle_lib as O
from tests import ristretto_ref as ref
from tests.test_gpu import CK, FULL, H, _check_ceremony, dec_str

pytestmark = pytest.mark.gpu

SHARDS = [[0], [0, 0], [0, 0, 0]]
L = ref.L


@pytest.fixture(scope="module", params=SHARDS, ids=lambda d: f"ws{len(d)}")
def mb(request):
    m = dkg_amd.MultiBackend(request.param)
    yield m
    m.close()


@pytest.fixture(scope="module")
def be():
    b = dkg_amd.Backend(0)
    yield b
    b.close()


def _dev(x):
    import torch

    return torch.frombuffer(bytearray(x or b"\0"), dtype=torch.uint8).to("cuda:0")


def _host(t):
    return bytes(t.cpu().numpy())


def _set_mode(m, mode):
    for i in range(len(m)):
        m.shard(i).set_key_comb(mode)


def _big(r):
    return {k: hashlib.sha256(getattr(r, k)).hexdigest() for k in ("dec2", "dec4", "final_share", "public_share")}


def _small(r):
    return {"mpk": r.mpk.hex(), "qualified": r.qualified, "reconstruct": r.reconstruct, "r2_error": r.r2_error,
            "r4_error": r.r4_error, "complaints2": r.complaints2, "n_qualified": r.n_qualified,
            "phase4_error": int(r.phase4_error)}


def _digest(r):
    return _big(r) | _small(r)


class Committee:
    """A seeded committee and its single-context full-mode runs: the device ceremony
    (ceremony_full_device: small outputs) and the receivers' run on the broadcasts the same context
    produced (share_gen + encrypt_shares -> ceremony_verify_full: every output)."""

    def __init__(self, be, n, t, seed):
        import torch

        self.n, self.t = n, t
        N = t + 1
        master = bytes([seed]) * 32
        be.env_init(t, n, CK)
        dev = torch.device("cuda", 0)
        ta = torch.empty(32 * n * N, dtype=torch.uint8, device=dev)
        tb = torch.empty_like(ta)
        tr = torch.empty(64 * n * n, dtype=torch.uint8, device=dev)
        be.dealer_coefficients_device(master, 1, 1, 0, n, t, ta.data_ptr(), tb.data_ptr())
        be.enc_randomness_device(master, 1, 1, 0, n, n, t, tr.data_ptr())
        self.a, self.b, self.r = _host(ta), _host(tb), _host(tr)
        self.sk, self.pk = be.member_keys(master, 1, n)
        self.small = _small(be.ceremony_full_device(ta.data_ptr(), tb.data_ptr(), tr.data_ptr(), self.sk, self.pk, n, t))
        self.E, self.A, s, sp = be.share_gen(self.a, self.b, n, n, t)
        self.e1, self.ct = be.encrypt_shares(self.pk, s, sp, self.r, n, n)
        self.full = be.ceremony_verify_full(self.E, self.A, self.e1, self.ct, self.sk, n, t)
        assert _small(self.full) == self.small and self.small["qualified"] == [1] * n

    def rank_bufs(self, ws, i):
        n, N = self.n, self.t + 1
        d0, d1 = dkg_amd.shard_range(n, ws, i)
        return [_dev(x[w * d0:w * d1]) for x, w in ((self.a, 32 * N), (self.b, 32 * N), (self.r, 64 * n))]


# ---------------------------------------------------------------- the libsodium fixtures
@pytest.mark.parametrize("name", ["full_n4_t1.json", "full_n10_t4.json"])
def test_shard_full_goldens_from_seeds(mb, golden, name):
    """From seeded coefficients, randomness and member keys (n = 4 over three shards: D = 1, 1, 2;
    n = 10: 3, 3, 4): the shards' encryption, decryption and checks give the fixture's outputs."""
    c = golden(name)
    n, t = c["n"], c["t"]
    if len(mb) > n:
        pytest.skip("more shards than dealers")
    mb.env_init(t, n, CK)
    master = H(c["master_seed"])
    a, b = dkg_amd.dealer_coefficients(master, c["ceremony"], 0, n, t)
    r = dkg_amd.enc_randomness(master, c["ceremony"], 0, n, n, t)
    assert r.hex() == c["enc_r"]
    res = mb.ceremony_full(a, b, r, H(c["member_sk"]), H(c["member_pk"]), n, t)
    assert res.mpk.hex() == c["mpk"] and res.qualified == c["qualified"]
    assert dec_str(res.dec2) == c["dec2"] and dec_str(res.dec4) == c["dec4"]
    assert res.final_share.hex() == c["final_share"] and res.public_share.hex() == c["public_share"]


@pytest.mark.parametrize("name", FULL)
def test_shard_full_goldens_from_broadcasts(mb, golden, name):
    """The receivers' side on the fixtures' ciphertexts, the tampered ones included: each shard decrypts
    its dealers' rows; every combined output as the fixture has it."""
    c = golden(name)
    n, t = c["n"], c["t"]
    if len(mb) > n:
        pytest.skip("more shards than dealers")
    mb.env_init(t, n, CK)
    r = mb.ceremony_verify_full(H(c["E"]), H(c["A"]), H(c["e1"]), H(c["ct"]), H(c["member_sk"]), n, t)
    assert r.E is None and r.s is None
    _check_ceremony(c, r, n)


def _shard_call(be, c, ws, i, with_ct=True):
    """Rank i of ws of the fixture's ceremony from seeds on `be`: (e1, ct) of its dealers."""
    import torch

    n, t = c["n"], c["t"]
    N = t + 1
    d0, d1 = dkg_amd.shard_range(n, ws, i)
    D = d1 - d0
    master = H(c["master_seed"])
    a, b = dkg_amd.dealer_coefficients(master, c["ceremony"], d0, D, t)
    ta, tb, tr = _dev(a), _dev(b), _dev(H(c["enc_r"])[64 * n * d0:64 * n * d1])
    u8 = dict(dtype=torch.uint8, device="cuda:0")
    o2, o4 = torch.empty(D * n, **u8), torch.empty(D * n, **u8)
    oA, op = torch.empty(D * 32, **u8), torch.empty(n * 32, **u8)
    e1, ct = torch.zeros(64 * D * n, **u8), torch.zeros(64 * D * n, **u8)
    assert len(a) == 32 * N * D
    ms = be.ceremony_shard_full_device(n, t, d0, d1, ta.data_ptr(), tb.data_ptr(), tr.data_ptr(), H(c["member_sk"]),
                                       H(c["member_pk"]), o2.data_ptr(), o4.data_ptr(), oA.data_ptr(), op.data_ptr(),
                                       e1.data_ptr() if with_ct else None, ct.data_ptr() if with_ct else None)
    assert ms > 0
    assert set(_host(o2)) <= {1, SELF}  # an honest shard: every receiver accepts
    return _host(e1), _host(ct), d0, d1


def test_shard_full_ciphertexts_per_rank(golden):
    """A rank's round-1 broadcast: d_e1 / d_ct of each of three ranks at n = 10 are rows [d0, d1) of the
    fixture's ciphertexts bit for bit, whichever comb multiplied (mode 1, mode 2), and last_key_comb
    reports it.  Mode 0: keys the context has not seen take radix 16; once their radix-2^10 tables are
    held, mode 0 keeps those."""
    c = golden("full_n10_t4.json")
    n, t = c["n"], c["t"]
    be = dkg_amd.Backend(0)
    try:
        be.env_init(t, n, CK)
        assert be.last_key_comb() == 0
        be.set_key_comb(0)
        _shard_call(be, c, 3, 0)
        assert be.last_key_comb() == 2  # fresh keys
        for mode in (1, 2):
            be.set_key_comb(mode)
            for i in range(3):
                e1, ct, d0, d1 = _shard_call(be, c, 3, i)
                assert e1.hex() == c["e1"][128 * n * d0:128 * n * d1], (mode, i)
                assert ct.hex() == c["ct"][128 * n * d0:128 * n * d1], (mode, i)
                assert be.last_key_comb() == mode
        be.set_key_comb(1)
        _shard_call(be, c, 3, 1, with_ct=False)
        be.set_key_comb(0)
        e1, ct, d0, d1 = _shard_call(be, c, 3, 2)
        assert be.last_key_comb() == 1  # the cached radix-2^10 set is kept
        assert e1.hex() == c["e1"][128 * n * d0:128 * n * d1] and ct.hex() == c["ct"][128 * n * d0:128 * n * d1]
    finally:
        be.close()


def test_shard_full_missing_row_through_the_exchange(be, golden):
    """One undecodable e1 item in a dealer of the LAST of three shards (n = 10: dealers 6..9): its round-2
    row is MISSING, it is disqualified without a complaint, and every combined output equals the
    single context's on the same input."""
    c = golden("full_n10_t4.json")
    n, t = c["n"], c["t"]
    bad, q, w = 8, 3, 1
    junk = H(golden("kat_group.json")["invalid_encodings"][0])
    e1 = bytearray(H(c["e1"]))
    k = 2 * (bad * n + q) + w
    e1[32 * k:32 * k + 32] = junk
    args = (H(c["E"]), H(c["A"]), bytes(e1), H(c["ct"]), H(c["member_sk"]), n, t)
    be.env_init(t, n, CK)
    want = be.ceremony_verify_full(*args)
    assert [want.dec2[bad * n + j] for j in range(n)] == [SELF if j == bad else MISSING for j in range(n)]
    m = dkg_amd.MultiBackend([0, 0, 0])
    try:
        m.env_init(t, n, CK)
        got = m.ceremony_verify_full(*args)
    finally:
        m.close()
    assert [got.dec2[bad * n + j] for j in range(n)] == [SELF if j == bad else MISSING for j in range(n)]
    assert got.qualified == [0 if i == bad else 1 for i in range(n)] and got.complaints2 == [0] * n
    assert _digest(got) == _digest(want)


# ---------------------------------------------------------------- shapes: lane groups, ragged shards
@pytest.fixture(scope="module")
def c130(be):
    return Committee(be, 130, 64, 0x41)


@pytest.mark.parametrize("mode", [1, 2])
def test_shard_full_lane_group_boundary_from_seeds(be, c130, mode):
    """n = 130, t = 64 over two shards, D = 65: the decryption's second 64-dealer group has one live
    lane, and a key's 130 radix-16 items end in a wave with two live lanes."""
    c = c130
    m = dkg_amd.MultiBackend([0, 0])
    try:
        m.env_init(c.t, c.n, CK)
        _set_mode(m, mode)
        got = m.ceremony_full(c.a, c.b, c.r, c.sk, c.pk, c.n, c.t)
        assert [m.shard(i).last_key_comb() for i in range(2)] == [mode, mode]
    finally:
        m.close()
    assert _small(got) == c.small
    assert _digest(got) == _digest(c.full)


def test_shard_full_lane_group_boundary_tampered(be, c130):
    """Tampered ciphertexts in dealer 64 (the lone lane of shard 0's second group), dealer 65 (shard 1's
    first lane) and dealer 129 (shard 1's lone lane): the receivers' rejections and everything that
    follows equal the single context's."""
    c = c130
    n, t = c.n, c.t
    ct = bytearray(c.ct)
    for i, q, w in ((64, 7, 1), (65, 129, 0), (129, 0, 1)):
        ct[32 * (2 * (i * n + q) + w) + 5] ^= 0x10
    be.env_init(t, n, CK)
    want = be.ceremony_verify_full(c.E, c.A, c.e1, bytes(ct), c.sk, n, t)
    assert want.qualified == [0 if i in (64, 65, 129) else 1 for i in range(n)]
    m = dkg_amd.MultiBackend([0, 0])
    try:
        m.env_init(t, n, CK)
        got = m.ceremony_verify_full(c.E, c.A, c.e1, bytes(ct), c.sk, n, t)
    finally:
        m.close()
    assert _digest(got) == _digest(want)


def test_shard_full_ragged_thirds(be):
    """n = 64, t = 31 over three shards (21, 21, 22 dealers), from seeds and from broadcasts."""
    c = Committee(be, 64, 31, 0x42)
    assert [dkg_amd.shard_range(64, 3, i) for i in range(3)] == [(0, 21), (21, 42), (42, 64)]
    m = dkg_amd.MultiBackend([0, 0, 0])
    try:
        m.env_init(c.t, c.n, CK)
        got = m.ceremony_full(c.a, c.b, c.r, c.sk, c.pk, c.n, c.t)
        got_v = m.ceremony_verify_full(c.E, c.A, c.e1, c.ct, c.sk, c.n, c.t)
    finally:
        m.close()
    assert _digest(got) == _digest(c.full) and _digest(got_v) == _digest(c.full)


@pytest.mark.parametrize("ws", [2, 3])
def test_shard_full_reconstruction_from_decrypted_shares(be, golden, ws):
    """Dealers accused in round 4 are reconstructed on the owning shard from the shares it DECRYPTED
    (dkg_ceremony_shard_recon_device with d_s = NULL): the fixture's shares under seeded keys and
    randomness give its reconstruction set, mpk and every other output."""
    c = golden("fault_recon_only_n10_t4.json")
    n, t = c["n"], c["t"]
    assert any(c["reconstruct"])
    master = H(c["master_seed"])
    be.env_init(t, n, CK)
    sk, pk = be.member_keys(master, c["ceremony"], n)
    r = dkg_amd.enc_randomness(master, c["ceremony"], 0, n, n, t)
    e1, ct = be.encrypt_shares(pk, H(c["s"]), H(c["s_prime"]), r, n, n)
    m = dkg_amd.MultiBackend([0] * ws)
    try:
        m.env_init(t, n, CK)
        got = m.ceremony_verify_full(H(c["E"]), H(c["A"]), e1, ct, sk, n, t)
    finally:
        m.close()
    _check_ceremony(c, got, n)


def test_shard_full_key_caches_follow_keys_and_kind(be):
    """Both kinds of comb are cached by the keys' bytes, separately: keys A mode 1, A mode 2, B mode 2,
    A mode 1, A mode 0 (n = 16, t = 7, two shards).  A stale comb of either kind would encrypt to other
    keys and every receiver would reject."""
    n, t = 16, 7
    be.env_init(t, n, CK)
    a, b = dkg_amd.dealer_coefficients(b"\x11" * 32, 0, 0, n, t)
    r = dkg_amd.enc_randomness(b"\x11" * 32, 0, 0, n, n, t)
    A, B = (be.member_keys(s, 0, n) for s in (b"\x21" * 32, b"\x22" * 32))
    m = dkg_amd.MultiBackend([0, 0])
    mpks = []
    try:
        m.env_init(t, n, CK)
        for (sk, pk), mode, kind in ((A, 1, 1), (A, 2, 2), (B, 2, 2), (A, 1, 1), (A, 0, 1)):
            _set_mode(m, mode)
            res = m.ceremony_full(a, b, r, sk, pk, n, t)
            assert res.qualified == [1] * n and res.n_qualified == n, (mode, kind)
            assert [m.shard(i).last_key_comb() for i in range(2)] == [kind, kind]
            mpks.append(res.mpk)
    finally:
        m.close()
    assert len(set(mpks)) == 1


def test_shard_full_radix16_recoding_edges_with_fewer_dealers_than_keys(be):
    """The radix-16 edge scalars (digits 8 / -8, carries through every window, the top digit) as
    encryption randomness with D = 3 dealers and n = 5 keys under the radix-16 comb: the ciphertexts
    equal the oracle's hybrid_encrypt."""
    rng = random.Random(23)
    D, n = 3, 5
    per = 2 * D * n
    k16 = EV.comb_scalars(4)
    sks = [rng.randrange(1, L) for _ in range(n)]
    pks = [O.base_mul(ref.sc(k)) for k in sks]
    be.set_key_comb(2)
    try:
        for c0 in range(0, len(k16), per):
            r = [k16[(c0 + i) % len(k16)] for i in range(per)]
            s = [rng.randrange(L) for _ in range(D * n)]
            sp = [rng.randrange(L) for _ in range(D * n)]
            cat = lambda xs: b"".join(ref.sc(x) for x in xs)  # noqa: E731
            e1, ct = be.encrypt_shares(b"".join(pks), cat(s), cat(sp), cat(r), D, n)
            assert be.last_key_comb() == 2
            for i in range(D):
                for q in range(n):
                    for w, msg in ((0, sp), (1, s)):
                        k = 2 * (i * n + q) + w
                        want = O.hybrid_encrypt(pks[q], ref.sc(r[k]), ref.sc(msg[i * n + q]))
                        assert (e1[32 * k:32 * k + 32], ct[32 * k:32 * k + 32]) == want, (c0, i, q, w)
    finally:
        be.set_key_comb(0)


# ---------------------------------------------------------------- the headline shape, once
def test_shard_full_n1024_matches_single_context(be):
    """n = 1024, t = 511 over two shards in mode 0, from host inputs and from per-shard device buffers,
    against one context's ceremony_full_device; an honest full-mode ceremony also decides and
    finalises exactly as the plaintext one."""
    import torch

    n, t = 1024, 511
    N = t + 1
    master = bytes(range(32))
    be.env_init(t, n, CK)
    dev = torch.device("cuda", 0)
    ta = torch.empty(32 * n * N, dtype=torch.uint8, device=dev)
    tb = torch.empty_like(ta)
    tr = torch.empty(64 * n * n, dtype=torch.uint8, device=dev)
    be.dealer_coefficients_device(master, 7, 1, 0, n, t, ta.data_ptr(), tb.data_ptr())
    be.enc_randomness_device(master, 7, 1, 0, n, n, t, tr.data_ptr())
    sk, pk = be.member_keys(master, 7, n)
    want = _small(be.ceremony_full_device(ta.data_ptr(), tb.data_ptr(), tr.data_ptr(), sk, pk, n, t))
    assert want["qualified"] == [1] * n
    a, b, r = _host(ta), _host(tb), _host(tr)
    m = dkg_amd.MultiBackend([0, 0])
    try:
        m.env_init(t, n, CK)
        plain = _big(m.ceremony(a, b, n, t))
        got = m.ceremony_full(a, b, r, sk, pk, n, t)
        assert _small(got) == want and _big(got) == plain
        assert [m.shard(i).last_key_comb() for i in range(2)] == [2, 2]  # cold keys: the cost rule
        bufs = []
        for i in range(2):
            d0, d1 = dkg_amd.shard_range(n, 2, i)
            bufs.append([ta[32 * N * d0:32 * N * d1], tb[32 * N * d0:32 * N * d1], tr[64 * n * d0:64 * n * d1]])
        got = m.ceremony_full_device(*([x[k].data_ptr() for x in bufs] for k in range(3)), sk, pk, n, t)
        assert _small(got) == want and _big(got) == plain
        ms = m.phase_ms()
        assert ms["shard_max"] >= ms["shard_min"] > 0
    finally:
        m.close()


# ---------------------------------------------------------------- arguments
def test_shard_full_rejects_bad_arguments(be, golden):
    import torch

    c = golden("full_n4_t1.json")
    n, t = c["n"], c["t"]
    be.env_init(t, n, CK)
    sk, pk = H(c["member_sk"]), H(c["member_pk"])
    z = torch.zeros(64 * n * n, dtype=torch.uint8, device="cuda:0")
    p = z.data_ptr()
    with pytest.raises(dkg_amd.DkgError):
        be.ceremony_shard_full_device(n, t, 0, 2, p, p, p, None, pk, p, p, p, p)  # NULL keys
    with pytest.raises(dkg_amd.DkgError):
        be.ceremony_shard_full_device(n, t, 0, 2, p, p, p, sk, None, p, p, p, p)
    with pytest.raises(dkg_amd.DkgError):
        be.ceremony_shard_verify_full_device(n, t, 0, 2, p, p, p, p, None, p, p, p, p)
    with pytest.raises(dkg_amd.DkgError):
        be.ceremony_shard_full_device(n, t, 2, 1, p, p, p, sk, pk, p, p, p, p)  # d1 < d0
    with pytest.raises(dkg_amd.DkgError):
        be.ceremony_shard_verify_full_device(n, t, 2, 1, p, p, p, p, sk, p, p, p, p)
    with pytest.raises(dkg_amd.DkgError):
        be.set_key_comb(3)
    with pytest.raises(dkg_amd.DkgError):
        be.set_key_comb(-1)
    a, b = dkg_amd.dealer_coefficients(H(c["master_seed"]), c["ceremony"], 0, n, t)
    r = H(c["enc_r"])
    m = dkg_amd.MultiBackend([0, 0, 0])
    try:
        m.env_init(0, 2, CK)
        with pytest.raises(dkg_amd.DkgError):
            m.ceremony_full(a, b, r, sk, pk, 2, 0)  # three shards, two dealers
        with pytest.raises(dkg_amd.DkgError):
            m.ceremony_verify_full(H(c["E"]), H(c["A"]), H(c["e1"]), H(c["ct"]), sk, 2, 0)
        m.env_init(t, n, CK)
        with pytest.raises(dkg_amd.DkgError):
            m.ceremony_full(a, b, r, None, pk, n, t)
        lib = _lib.lib()
        keep = ctypes.create_string_buffer(32 * n * n)
        for call in (lambda o: lib.dkg_multi_ceremony_run_full(m._m, n, t, a, b, r, sk, pk, ctypes.byref(o)),
                     lambda o: lib.dkg_multi_ceremony_verify_full(m._m, n, t, H(c["E"]), H(c["A"]), H(c["e1"]),
                                                                  H(c["ct"]), sk, ctypes.byref(o))):
            o, bufs = m._out(n, t)
            o.s = ctypes.cast(keep, ctypes.c_void_p)  # the shares stay on the shards' devices
            with pytest.raises(dkg_amd.DkgError):
                m._check(call(o))
        assert m.ceremony_full(a, b, r, sk, pk, n, t).mpk.hex() == c["mpk"]  # and the context still works
    finally:
        m.close()
