"""Full (encrypted-share) mode for batches of ceremonies: dkg_member_keys_batch, dkg_encrypt_shares_batch,
dkg_decrypt_shares_batch, dkg_ceremony_batch_full_device, dkg_ceremony_batch_verify_full.

The references are the CPU oracle (tests/oracle_lib.py), the golden fixtures and the single-ceremony
entry points (member_keys, encrypt_shares, ceremony_verify_full, ceremony_full_device); comparisons
are bit-exact.  Row c*n + i of every array is dealer i of ceremony c; keys are [B][n][32].
"""
import ctypes
import random

import pytest

import dkg_amd
from dkg_amd import MISSING, SELF, _lib
from tests import oracle_lib as O
from tests.test_gpu import _check_batch_member

pytestmark = pytest.mark.gpu

H = bytes.fromhex
L = 2**252 + 27742317777372353535851937790883648493
CK = b"Example of a shared string."
# partial wave, exactly one wave of dealers, one wave plus a one-lane tail, several keys' worth of work
SHAPES = [(3, 5), (2, 64), (2, 65), (5, 10)]
RESULT_FIELDS = ("mpk", "n_qualified", "phase4_error", "qualified", "r2_error", "r4_error", "complaints2", "reconstruct",
                 "final_share", "public_share", "dec2", "dec4")


@pytest.fixture(scope="module")
def be():
    b = dkg_amd.Backend(0)
    yield b
    b.close()


def sc(v):
    return (v % L).to_bytes(32, "little")


_cases = {}


def case(be, B, n):
    """Random inputs of one shape and their batched encryption, computed once per module."""
    if (B, n) in _cases:
        return _cases[(B, n)]
    rng = random.Random(1000 * B + n)
    V = B * n
    sks = [rng.randrange(1, L) for _ in range(V)]
    sks[0], sks[V - 1] = 1, L - 1  # the keys g*1 and g*(l-1)
    sk = b"".join(sc(k) for k in sks)
    pk = be.fixed_base_batch(sk)
    assert pk[:32] == O.base_mul(sc(1)) and pk[-32:] == O.base_mul(sc(L - 1))
    s = b"".join(sc(rng.randrange(L)) for _ in range(V * n))
    sp = b"".join(sc(rng.randrange(L)) for _ in range(V * n))
    rs = [rng.randrange(L) for _ in range(2 * V * n)]
    rs[0], rs[1], rs[2] = 0, 1, L - 1              # under the key g*1
    rs[-1], rs[-2], rs[-3] = 0, 1, L - 1           # the last items, under g*(l-1)
    rs[2 * n * n + 3] = 0                          # and one in the second ceremony
    r = b"".join(sc(v) for v in rs)
    e1, ct = be.encrypt_shares_batch(pk, s, sp, r, B, n)
    _cases[(B, n)] = dict(sk=sk, pk=pk, s=s, sp=sp, r=r, e1=e1, ct=ct)
    return _cases[(B, n)]


def test_member_keys_batch(be, golden):
    c = golden("full_n10_t4.json")
    master, c0, B, n = H(c["master_seed"]), c["ceremony"], 3, c["n"]
    assert c0 == 4
    sk, pk = be.member_keys_batch(master, c0, B, n)
    assert len(sk) == len(pk) == 32 * B * n
    for k in range(B):
        rsk, rpk = be.member_keys(master, c0 + k, n)
        assert sk[32 * n * k:32 * n * (k + 1)] == rsk and pk[32 * n * k:32 * n * (k + 1)] == rpk
    assert sk[:32 * n].hex() == c["member_sk"] and pk[:32 * n].hex() == c["member_pk"]


@pytest.mark.parametrize("B,n", SHAPES)
def test_encrypt_batch_equals_single_and_oracle(be, B, n):
    d = case(be, B, n)
    row, key = 64 * n * n, 32 * n  # ciphertext bytes and key bytes per ceremony
    for c in range(B):
        pair = slice(32 * n * n * c, 32 * n * n * (c + 1))
        e1, ct = be.encrypt_shares(d["pk"][key * c:key * (c + 1)], d["s"][pair], d["sp"][pair],
                                   d["r"][row * c:row * (c + 1)], n, n)
        assert d["e1"][row * c:row * (c + 1)] == e1, c
        assert d["ct"][row * c:row * (c + 1)] == ct, c
    rng = random.Random(7)
    sample = [(c, i, q, w) for c in range(B) for (i, q) in ((0, 0), (n - 1, n - 1)) for w in (0, 1)]
    sample += [(0, 0, 1, 0), (1, 0, 1, 1)]  # the randomness 1 / l-1 under g*1, the 0 of the second ceremony
    sample += [(rng.randrange(B), rng.randrange(n), rng.randrange(n), rng.randrange(2)) for _ in range(8)]
    for c, i, q, w in sample:
        p = (c * n + i) * n + q
        k = 2 * p + w
        msg = (d["sp"], d["s"])[w][32 * p:32 * p + 32]
        pkq = d["pk"][32 * (c * n + q):32 * (c * n + q) + 32]
        assert O.hybrid_encrypt(pkq, d["r"][32 * k:32 * k + 32], msg) == \
            (d["e1"][32 * k:32 * k + 32], d["ct"][32 * k:32 * k + 32]), (c, i, q, w)


@pytest.mark.parametrize("B,n", SHAPES)
def test_decrypt_batch(be, B, n):
    d = case(be, B, n)
    s, sp, ok = be.decrypt_shares_batch(d["sk"], d["e1"], d["ct"], B, n)
    assert s == d["s"] and sp == d["sp"] and ok == b"\x01" * (2 * B * n * n)
    # the keys of the next ceremony do not decrypt this one's shares
    rot = d["sk"][32 * n:] + d["sk"][:32 * n]
    s2, sp2, _ = be.decrypt_shares_batch(rot, d["e1"], d["ct"], B, n)
    assert s2 != d["s"] and sp2 != d["sp"]
    # an e1 that does not decode is flagged for its own item only
    bad = next(x for x in (b"\xff" * 32, b"\x01" + b"\x00" * 31, b"\x02" + b"\x00" * 31) if be.points_valid(x) == b"\x00")
    k = 2 * ((1 * n + n - 1) * n + 1) + 1  # ceremony 1, its last dealer, recipient 1, the share
    e1 = d["e1"][:32 * k] + bad + d["e1"][32 * k + 32:]
    _, _, ok3 = be.decrypt_shares_batch(d["sk"], e1, d["ct"], B, n)
    assert ok3 == b"\x01" * k + b"\x00" + b"\x01" * (2 * B * n * n - k - 1)


def _device_inputs(be, master, c0, B, n, t):
    import torch

    dev = torch.device("cuda", 0)
    N = t + 1
    ta = torch.empty(32 * B * n * N, dtype=torch.uint8, device=dev)
    tb = torch.empty_like(ta)
    tr = torch.empty(64 * B * n * n, dtype=torch.uint8, device=dev)
    be.dealer_coefficients_device(master, c0, B, 0, n, t, ta.data_ptr(), tb.data_ptr())
    be.enc_randomness_device(master, c0, B, 0, n, n, t, tr.data_ptr())
    return ta, tb, tr


def _fields(r):
    return {k: (list(getattr(r, k)) if k == "complaints2" else getattr(r, k)) for k in RESULT_FIELDS}


def test_chunk_boundaries(be, golden):
    """Chunks of 2 and of 1 ceremony inside a batch of 5 give the automatic setting's outputs."""
    B, n, t = 5, 10, 4
    d = case(be, B, n)
    master = H(golden("full_n10_t4.json")["master_seed"])
    be.env_init(t, n, CK)
    ta, tb, tr = _device_inputs(be, master, 4, B, n, t)
    sk, pk = be.member_keys_batch(master, 4, B, n)
    outs = []
    try:
        for chunk in (0, 2, 1):
            be.set_batch_full_chunk(chunk)
            enc = be.encrypt_shares_batch(d["pk"], d["s"], d["sp"], d["r"], B, n)
            dec = be.decrypt_shares_batch(d["sk"], d["e1"], d["ct"], B, n)
            r = dkg_amd.ceremony_batch_full_device(be, B, n, t, ta.data_ptr(), tb.data_ptr(), tr.data_ptr(), sk, pk,
                                                   big=True)
            outs.append((enc, dec, _fields(r)))
    finally:
        be.set_batch_full_chunk(0)
    assert outs[0][0] == (d["e1"], d["ct"]) and outs[0][1][:2] == (d["s"], d["sp"])
    assert outs[0][2]["n_qualified"] == [n] * B
    assert outs[1] == outs[0] and outs[2] == outs[0]


def _tampered_ceremony(be, master, ceremony, n, t, bad_e1=None):
    """A ceremony built through the single-ceremony calls with keys of its own and one flipped
    ciphertext byte (and optionally an undecodable e1): (E, A, e1, ct, sk)."""
    a, b = dkg_amd.dealer_coefficients(master, ceremony, 0, n, t)
    E, A, s, sp = be.share_gen(a, b, n, n, t)
    sk, pk = be.member_keys(master, ceremony, n)
    e1, ct = be.encrypt_shares(pk, s, sp, dkg_amd.enc_randomness(master, ceremony, 0, n, n, t), n, n)
    k = 2 * (2 * n + 7) + 1  # dealer 2 -> receiver 7, the share
    ct = ct[:32 * k + 5] + bytes([ct[32 * k + 5] ^ 0x40]) + ct[32 * k + 6:]
    if bad_e1 is not None:
        k = 2 * (5 * n + 3)  # dealer 5 -> receiver 3, the randomness
        e1 = e1[:32 * k] + bad_e1 + e1[32 * k + 32:]
    return E, A, e1, ct, sk


def _same_as_single(d, ref, n):
    assert d["mpk"] == ref.mpk and d["n_qualified"] == ref.n_qualified and d["phase4_error"] == ref.phase4_error
    for k in ("qualified", "r2_error", "r4_error", "complaints2", "reconstruct"):
        assert list(d[k]) == getattr(ref, k), k
    for k in ("final_share", "public_share", "dec2", "dec4"):
        assert d[k] == getattr(ref, k), k


@pytest.mark.parametrize("undecodable", [False, True])
def test_batch_verify_full_goldens(be, golden, undecodable):
    n, t = 10, 4
    cs = [golden("full_n10_t4.json"), golden("full_faults_n10_t4.json"), golden("full_n10_t4.json")]
    assert all((c["n"], c["t"]) == (n, t) for c in cs)
    be.env_init(t, n, CK)
    bad = b"\xff" * 32 if undecodable else None
    if undecodable:
        assert be.points_valid(bad) == b"\x00"
    own = _tampered_ceremony(be, H(cs[0]["master_seed"]), 9, n, t, bad)
    assert own[4] != H(cs[0]["member_sk"])  # keys of its own
    ref = be.ceremony_verify_full(*own, n, t)
    parts = [[H(c[k]) for c in cs] + [own[j]] for j, k in enumerate(("E", "A", "e1", "ct", "member_sk"))]
    E, A, e1, ct, sk = (b"".join(p) for p in parts)
    r = dkg_amd.ceremony_batch_verify_full(be, 4, n, t, E, A, e1, ct, sk)
    sz = 32 * n * n
    for k, c in enumerate(cs):
        _check_batch_member(c, r.ceremony(k), n)
        assert r.s[sz * k:sz * (k + 1)].hex() == c["s"] and r.s_prime[sz * k:sz * (k + 1)].hex() == c["s_prime"]
    d = r.ceremony(3)
    _same_as_single(d, ref, n)
    assert r.s[3 * sz:] == ref.s and r.s_prime[3 * sz:] == ref.s_prime
    assert d["qualified"][2] == 0 and d["complaints2"][7] == 1  # the flipped ciphertext byte: a complaint
    if undecodable:
        row = bytes(SELF if j == 5 else MISSING for j in range(n))  # every receiver but the dealer itself
        assert d["dec2"][5 * n:6 * n] == row and d["qualified"][5] == 0 and d["complaints2"][3] == 0
    else:
        assert MISSING not in d["dec2"]


def test_batch_full_device_ceremony(be, golden):
    c = golden("full_n10_t4.json")
    B, n, t, c0 = 3, c["n"], c["t"], c["ceremony"]
    master = H(c["master_seed"])
    be.env_init(t, n, CK)
    ta, tb, tr = _device_inputs(be, master, c0, B, n, t)
    sk, pk = be.member_keys_batch(master, c0, B, n)
    r = dkg_amd.ceremony_batch_full_device(be, B, n, t, ta.data_ptr(), tb.data_ptr(), tr.data_ptr(), sk, pk, big=True)
    assert r.mpk[0].hex() == c["mpk"] and r.ceremony(0)["qualified"] == c["qualified"]
    _check_batch_member(c, r.ceremony(0), n)
    N = t + 1
    for k in (1, 2):
        ks, kp = sk[32 * n * k:32 * n * (k + 1)], pk[32 * n * k:32 * n * (k + 1)]
        a, b = ta[32 * n * N * k:32 * n * N * (k + 1)], tb[32 * n * N * k:32 * n * N * (k + 1)]
        rr = tr[64 * n * n * k:64 * n * n * (k + 1)]
        d = r.ceremony(k)
        # the single device ceremony on this ceremony's own coefficients, randomness and keys
        one = be.ceremony_full_device(a.data_ptr(), b.data_ptr(), rr.data_ptr(), ks, kp, n, t)
        assert d["mpk"] == one.mpk and d["qualified"] == one.qualified and d["n_qualified"] == one.n_qualified == n
        assert list(d["complaints2"]) == one.complaints2 and d["reconstruct"] == one.reconstruct
        # its large outputs through the single receiver side, from ciphertexts of the single encryption
        ha, hb = dkg_amd.dealer_coefficients(master, c0 + k, 0, n, t)
        assert bytes(a.cpu().numpy()) == ha
        E, A, s, sp = be.share_gen(ha, hb, n, n, t)
        e1, ct = be.encrypt_shares(kp, s, sp, dkg_amd.enc_randomness(master, c0 + k, 0, n, n, t), n, n)
        _same_as_single(d, be.ceremony_verify_full(E, A, e1, ct, ks, n, t), n)
    # protocol order (round 4 after round 3, the whole round 1 first) gives the same batch
    be.set_overlap(False)
    try:
        r2 = dkg_amd.ceremony_batch_full_device(be, B, n, t, ta.data_ptr(), tb.data_ptr(), tr.data_ptr(), sk, pk, big=True)
    finally:
        be.set_overlap(True)
    assert _fields(r2) == _fields(r)


def test_batch_full_device_n64(be):
    import torch

    B, n, t = 2, 64, 31
    N = t + 1
    master = bytes(range(32))
    be.env_init(t, n, CK)
    ta, tb, tr = _device_inputs(be, master, 0, B, n, t)
    sk, pk = be.member_keys_batch(master, 0, B, n)
    r = dkg_amd.ceremony_batch_full_device(be, B, n, t, ta.data_ptr(), tb.data_ptr(), tr.data_ptr(), sk, pk)
    assert r.n_qualified == [n] * B and r.qualified == b"\x01" * (B * n) and r.phase4_error == b"\x00" * B
    a0 = bytes(ta.view(B * n, N * 32)[:, :32].contiguous().cpu().numpy())
    for c in range(B):
        secret = sum(int.from_bytes(a0[32 * i:32 * i + 32], "little") for i in range(c * n, (c + 1) * n)) % L
        assert r.mpk[c] == O.base_mul(sc(secret))
    assert torch.cuda.is_available()


def test_batch_full_arguments(be):
    n, t = 10, 4
    be.env_init(t, n, CK)
    assert be.member_keys_batch(b"\x01" * 32, 0, 0, n) == (b"", b"")
    assert be.encrypt_shares_batch(b"", b"", b"", b"", 0, n) == (b"", b"")
    assert be.decrypt_shares_batch(b"", b"", b"", 0, n) == (b"", b"", b"")
    lib = _lib.lib()
    o, _bufs = dkg_amd.api._batch_out(1, n, False)
    one = ctypes.create_string_buffer(32 * n * n * 4)
    vp = ctypes.c_void_p
    assert lib.dkg_ceremony_batch_full_device(be.ctx, 0, n, t, vp(0), vp(0), vp(0), one, one, ctypes.byref(o)) == _lib.DKG_OK
    assert lib.dkg_ceremony_batch_verify_full(be.ctx, 0, n, t, one, one, one, one, one, ctypes.byref(o), None, None) == _lib.DKG_OK
    # a NULL sk is an argument error, whatever B is
    assert lib.dkg_ceremony_batch_full_device(be.ctx, 1, n, t, vp(0), vp(0), vp(0), None, one,
                                              ctypes.byref(o)) == _lib.DKG_E_ARG
    assert lib.dkg_ceremony_batch_verify_full(be.ctx, 1, n, t, one, one, one, one, None, ctypes.byref(o), None,
                                              None) == _lib.DKG_E_ARG
    assert lib.dkg_decrypt_shares_batch(be.ctx, 1, n, None, one, one, one, one, None) == _lib.DKG_E_ARG
    assert lib.dkg_encrypt_shares_batch(be.ctx, 1, n, None, one, one, one, one, one) == _lib.DKG_E_ARG
    assert lib.dkg_member_keys_batch(be.ctx, b"\x01" * 32, 0, 1, n, None, one) == _lib.DKG_E_ARG
    # a recipient key that does not decode: DKG_E_DECODE, as dkg_encrypt_shares
    bad = b"\xff" * 32
    assert be.points_valid(bad) == b"\x00"
    pk = be.fixed_base_batch(b"".join(sc(k + 1) for k in range(2 * n)))
    z = b"\x00" * (32 * 2 * n * n)
    with pytest.raises(dkg_amd.DkgError) as ei:
        be.encrypt_shares_batch(pk[:32 * (n + 3)] + bad + pk[32 * (n + 4):], z, z, z + z, 2, n)
    assert ei.value.code == _lib.DKG_E_DECODE
    # t >= (n + 1) / 2 is rejected as in the neighbouring calls
    assert lib.dkg_ceremony_batch_verify_full(be.ctx, 1, n, 5, one, one, one, one, one, ctypes.byref(o), None,
                                              None) == _lib.DKG_E_ARG
