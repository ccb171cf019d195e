"""Structured edge inputs through the kernels: the signed comb recodings (radix 2^19 for g and h,
2^10 for the member keys, 16 for the batched encryption), the width-4 window chain of the decryption,
the lazy Horner of the share evaluation, the Ristretto decoder and the MSM's workgroup sizes.

Expected values come from the big-integer reference tests/ristretto_ref.py (computed once per module
and shared), and from the C oracle where Blake2b / ChaCha20 are involved; tests/test_edge_vectors.py
shows on the CPU that the two agree on every vector used here and that the vectors hold the rare
cases.  Byte equality throughout.

The decryption's chain is the width-4 window one (k_dec_mul_w4 / k_bdec_mul_w4): the bitwise NAF chain
k_dec_mul is a build-time alternative (-DDKG_DEC_NAF) that the shipped library never launches.
"""
import random

import pytest

import dkg_amd
from dkg_amd import ACCEPT, MISSING, REJECT, SELF, SKIPPED
from tests import edge_vectors as EV
from tests import oracle_lib as O
from tests import ristretto_ref as ref

pytestmark = pytest.mark.gpu

H = bytes.fromhex
L = ref.L
CK = b"Example of a shared string."


@pytest.fixture(scope="module")
def be():
    b = dkg_amd.Backend(0)
    yield b
    b.close()


class Expected:
    """The module's reference values: g*k and h*k by big-integer arithmetic, each computed once."""

    def __init__(self, golden):
        lib = dkg_amd.lib()
        self.B_gh = EV.comb_radix(lib.dkg_fixed_base_windows())
        self.B_key = EV.comb_radix(lib.dkg_key_comb_windows())
        self.k_gh = EV.comb_scalars(self.B_gh)
        self.k_key = EV.comb_scalars(self.B_key)
        self.k16 = EV.comb_scalars(4)
        self.naf = EV.naf_scalars()
        kat = golden("kat_group.json")
        self.h_bytes = H(kat["hash_to_group"][0]["P"])  # the commitment key of CK
        self.caller_bytes = H(kat["mul"][0]["P"])
        self.bad_fixture = [H(x) for x in kat["invalid_encodings"]]
        self._tab = {"g": ref.doublings(ref.BASE), "h": ref.doublings(ref.decode(self.h_bytes)),
                     "caller": ref.doublings(ref.decode(self.caller_bytes))}
        self._memo = {}

    def mul(self, base, k):
        k %= L
        if (base, k) not in self._memo:
            self._memo[base, k] = ref.mul_doublings(k, self._tab[base])
        return self._memo[base, k]

    def g(self, k):
        return ref.encode(self.mul("g", k))

    def commit(self, a, b):
        """E = h*b + g*a (committee.rs:151-159)."""
        return ref.encode(ref.add(self.mul("g", a), self.mul("h", b)))


@pytest.fixture(scope="module")
def ex(golden):
    return Expected(golden)


def sc(k):
    return ref.sc(k)


def cat(ks):
    return b"".join(sc(k) for k in ks)


def chunks(b, size=32):
    return [b[i:i + size] for i in range(0, len(b), size)]


def cycle_to(xs, count):
    return [xs[i % len(xs)] for i in range(count)]


# ---------------------------------------------------------------- fixed base (k_fixed_base, radix 2^19)
@pytest.mark.parametrize("base", ["g", "h", "caller"])
def test_fixed_base_comb_edges(be, ex, base):
    """Every window's edge digits through the comb of the generator, of h and of a caller's base;
    k + l and 2^256 - 1 are read as Scalar::from_bits reads them."""
    assert be.env_init(4, 10, CK) == ex.h_bytes
    arg = {"g": None, "h": ex.h_bytes, "caller": ex.caller_bytes}[base]
    want = [ref.encode(ex.mul(base, k)) for k in ex.k_gh]
    assert chunks(be.fixed_base_batch(cat(ex.k_gh), base=arg)) == want
    shifted = b"".join((k + L).to_bytes(32, "little") for k in ex.k_gh)
    assert chunks(be.fixed_base_batch(shifted, base=arg)) == want
    top = b"\xff" * 32
    assert be.fixed_base_batch(top, base=arg) == ref.encode(ex.mul(base, ref.from_bits(top)))


# ---------------------------------------------------------------- commitments (k_commit, k_commit_pm)
@pytest.mark.parametrize("n,t", [(16, 7), (64, 31)])
def test_share_gen_comb_edges(be, ex, n, t):
    """k_commit: a = the edge scalars, b = the same list reversed; E, A, s and s' against the reference."""
    be.env_init(t, n, CK)
    N = t + 1
    D = -(-len(ex.k_gh) // N)
    a = cycle_to(ex.k_gh, D * N)
    b = cycle_to(ex.k_gh[::-1], D * N)
    E, A, s, sp = be.share_gen(cat(a), cat(b), D, n, t)
    assert chunks(A) == [ex.g(k) for k in a]
    assert chunks(E) == [ex.commit(x, y) for x, y in zip(a, b)]
    rows = lambda c: cat(ref.poly_eval(c[N * i:N * i + N], j + 1) for i in range(D) for j in range(n))  # noqa: E731
    assert s == rows(a) and sp == rows(b)


def test_batch_commitments_comb_edges(be, ex):
    """k_commit_pm: the batched ceremonies compute their commitments straight into the verification's
    table (share_gen never takes that kernel), so the edge coefficients go through
    dkg_ceremony_batch_device.  A wrong E or A entry fails its dealer's checks, a wrong A_i0 the master
    key; final and public shares against the reference."""
    import torch

    n, t = 16, 7
    N = t + 1
    B = -(-len(ex.k_gh) // (n * N))
    assert B == 2
    be.env_init(t, n, CK)
    a = cycle_to(ex.k_gh, B * n * N)
    b = cycle_to(ex.k_gh[::-1], B * n * N)
    dev = torch.device("cuda", 0)
    ta = torch.frombuffer(bytearray(cat(a)), dtype=torch.uint8).to(dev)
    tb = torch.frombuffer(bytearray(cat(b)), dtype=torch.uint8).to(dev)
    r = dkg_amd.ceremony_batch_device(be, B, n, t, ta.data_ptr(), tb.data_ptr(), big=True)
    honest = bytes(SELF if i == j else ACCEPT for i in range(n) for j in range(n))
    for c in range(B):
        d = r.ceremony(c)
        assert d["dec2"] == honest and d["dec4"] == honest and d["qualified"] == [1] * n
        rows = [a[(c * n + i) * N:(c * n + i + 1) * N] for i in range(n)]
        mpk = ref.IDENTITY
        for row in rows:
            mpk = ref.add(mpk, ex.mul("g", row[0]))
        assert d["mpk"] == ref.encode(mpk)
        final = [sum(ref.poly_eval(row, j + 1) for row in rows) % L for j in range(n)]
        assert d["final_share"] == cat(final)
        assert chunks(d["public_share"]) == [ex.g(k) for k in final]


# ---------------------------------------------------------------- checks (k_check, k_check_both, interpolation)
def _edge_ceremony(ex, t):
    """n dealers, dealer i's shares to receiver (i + 1) % n being edge scalars: (E, A, s, s', pairs)."""
    rng = random.Random(100 + t)
    edges = ex.k_gh + ex.k_key[:6]
    n = len(edges)
    E, A, s, sp, pairs = [], [], [], [], []
    for i in range(n):
        j = (i + 1) % n
        fa = EV.share_at(edges[i], j + 1, t, rng, pool=ex.k_gh)
        fb = EV.share_at(edges[n - 1 - i], j + 1, t, rng, pool=ex.k_gh)
        E += [ex.commit(x, y) for x, y in zip(fa, fb)]
        A += [ex.g(x) for x in fa]
        s += [ref.poly_eval(fa, x) for x in range(1, n + 1)]
        sp += [ref.poly_eval(fb, x) for x in range(1, n + 1)]
        assert s[i * n + j] == edges[i] and sp[i * n + j] == edges[n - 1 - i]
        pairs.append((i, j))
    return n, b"".join(E), b"".join(A), s, sp, pairs


@pytest.fixture(scope="module")
def edge_ceremonies(ex):
    return {t: _edge_ceremony(ex, t) for t in (0, 2)}


@pytest.mark.parametrize("tamper", [False, True])
@pytest.mark.parametrize("t", [0, 2])
def test_checks_comb_edges(be, ex, edge_ceremonies, t, tamper):
    """One dealer per edge scalar: the share and the randomness its receiver checks are edge scalars.
    Honest: every pair ACCEPT.  With e + 1 in place of every edge share: exactly those pairs REJECT
    (in a ceremony that disqualifies every dealer, so round 4 is SKIPPED throughout)."""
    n, E, A, s, sp, pairs = edge_ceremonies[t]
    assert n == 190 and be.env_init(t, n, CK) == ex.h_bytes
    s = list(s)
    if tamper:
        for i, j in pairs:
            s[i * n + j] = (s[i * n + j] + 1) % L
    s, sp = cat(s), cat(sp)
    bad = set(pairs) if tamper else set()
    want = bytes(SELF if i == j else REJECT if (i, j) in bad else ACCEPT for i in range(n) for j in range(n))
    want4 = bytes(SELF if i == j else SKIPPED for i in range(n) for j in range(n)) if tamper else want
    assert be.verify_pairs(n, t, 2, 0, n, E, s, sp) == want
    assert be.verify_pairs(n, t, 4, 0, n, A, s) == want
    V = len(ex.k_gh)  # a dealer sub-range: the comb scalars' dealers alone
    N = t + 1
    assert be.verify_pairs(n, t, 2, 3, V, E[32 * N * 3:32 * N * V], s[32 * n * 3:32 * n * V],
                           sp[32 * n * 3:32 * n * V]) == want[n * 3:n * V]
    try:
        for check in (0, 1):
            for field in (1, 2):
                for overlap in (True, False):
                    be.set_check(check)
                    be.set_field_mode(field)
                    be.set_overlap(overlap)
                    r = be.ceremony_verify(E, A, s, sp, n, t)
                    assert r.dec2 == want and r.dec4 == want4, (check, field, overlap)
                    assert r.qualified == [0 if tamper else 1] * n
        be.set_check(0)
        be.set_field_mode(0)
        for overlap in (True, False):
            be.set_overlap(overlap)
            be.set_verify_mode(1)
            r = be.ceremony_verify(E, A, s, sp, n, t)
            assert r.dec2 == want and r.dec4 == want4, ("interp", overlap)
    finally:
        be.set_check(0)
        be.set_field_mode(0)
        be.set_overlap(True)
        be.set_verify_mode(0)


# ---------------------------------------------------------------- full mode (k_enc_mul, k_benc_mul, w4 chains)
def _members(ex, sks):
    """Keys sorted by public-key bytes, as dkg_member_keys returns them: (sk, pk) lists of bytes."""
    keyed = sorted((ex.g(k), sc(k)) for k in sks)
    return [s for _, s in keyed], [p for p, _ in keyed]


def _oracle_ciphertexts(pks, n, rows, s, sp, r, key_row=lambda i: 0):
    """hybrid_encrypt of every item on the CPU: item 2 (i n + q) + w carries s' (w = 0) or s (w = 1)
    of dealer row i to recipient q, under the key pks[key_row(i)][q]."""
    e1, ct = [], []
    for i in range(rows):
        for q in range(n):
            for w, msg in ((0, sp), (1, s)):
                k = 2 * (i * n + q) + w
                a, b = O.hybrid_encrypt(pks[key_row(i)][q], sc(r[k]), sc(msg[i * n + q]))
                e1.append(a)
                ct.append(b)
    return e1, ct


def test_full_mode_single_comb_and_window_edges(be, ex):
    """Member keys sk = the NAF / wNAF edge scalars (among them 0: the identity as a key), encryption
    randomness over the edge scalars of both comb radices.  e1 = g*r against the reference, (e1, ct)
    against the oracle; the decryption runs on the ORACLE's ciphertexts, so that an error cannot
    cancel against the device's encryption."""
    rng = random.Random(21)
    sks, pks = _members(ex, ex.naf)
    n = len(sks)
    rs = ex.k_gh + ex.k_key
    D = -(-len(rs) // (2 * n))
    r = cycle_to(rs, 2 * D * n)
    s = [rng.randrange(L) for _ in range(D * n)]
    sp = [rng.randrange(L) for _ in range(D * n)]
    want_e1, want_ct = _oracle_ciphertexts([pks], n, D, s, sp, r)
    assert want_e1 == [ex.g(k) for k in r]
    e1, ct = be.encrypt_shares(b"".join(pks), cat(s), cat(sp), cat(r), D, n)
    assert chunks(e1) == want_e1
    assert chunks(ct) == want_ct
    ds, dsp, ok = be.decrypt_shares(b"".join(sks), b"".join(want_e1), b"".join(want_ct), D, n)
    assert ds == cat(s) and dsp == cat(sp) and set(ok) == {1}


def test_full_mode_batch_comb_and_window_edges(be, ex):
    """The batched path: per-ceremony keys (radix-16 combs built per key, k_benc_mul) with the radix-16
    edge scalars as randomness, and the batched width-4 chain (k_bdec_mul_w4) on the oracle's
    ciphertexts."""
    rng = random.Random(22)
    keys = ex.naf + [rng.randrange(L) for _ in range(len(ex.naf) % 2)]
    B, n = 2, len(keys) // 2
    members = [_members(ex, keys[c * n:(c + 1) * n]) for c in range(B)]
    sks, pks = [m[0] for m in members], [m[1] for m in members]
    items = 2 * B * n * n
    assert items >= len(ex.k16)
    r = cycle_to(ex.k16, items)
    s = [rng.randrange(L) for _ in range(B * n * n)]
    sp = [rng.randrange(L) for _ in range(B * n * n)]
    want_e1, want_ct = _oracle_ciphertexts(pks, n, B * n, s, sp, r, key_row=lambda i: i // n)
    assert want_e1 == [ex.g(k) for k in r]
    pk_all, sk_all = b"".join(b"".join(p) for p in pks), b"".join(b"".join(k) for k in sks)
    e1, ct = be.encrypt_shares_batch(pk_all, cat(s), cat(sp), cat(r), B, n)
    assert chunks(e1) == want_e1
    assert chunks(ct) == want_ct
    ds, dsp, ok = be.decrypt_shares_batch(sk_all, b"".join(want_e1), b"".join(want_ct), B, n)
    assert ds == cat(s) and dsp == cat(sp) and set(ok) == {1}


# ---------------------------------------------------------------- complaint proofs
def test_complaint_proofs_edges(be, ex):
    """Proofs of misbehaviour with sk = the NAF / wNAF edge scalars and edge scalars as nonces: byte
    for byte the oracle's, from the host-driven primitive and from the device batch; valid complaints
    read 0, and 1 once a response is incremented -- in the per-complaint and the batched verification."""
    rng = random.Random(31)
    t = 2
    h = be.env_init(t, len(ex.naf), CK)
    assert h == ex.h_bytes
    n = len(ex.naf)
    sks = [sc(k) for k in ex.naf]
    pks = [ex.g(k) for k in ex.naf]
    C = len(ex.k_gh) // 2
    accuser = [b % n + 1 for b in range(C)]
    accused = [(b + 1) % n + 1 for b in range(C)]
    # commitments that the decrypted shares do not open: the complaints are justified
    Erows = [b"".join(ex.g(rng.choice(ex.k_gh)) for _ in range(t + 1)) for _ in range(n)]
    enc, w, want = [], [], []
    for b in range(C):
        pk = pks[accuser[b] - 1]
        e1r, ctr = O.hybrid_encrypt(pk, sc(rng.randrange(L)), sc(rng.randrange(L)))
        e1s, cts = O.hybrid_encrypt(pk, sc(rng.randrange(L)), sc(rng.randrange(L)))
        enc.append(e1r + ctr + e1s + cts)
        w.append(sc(ex.k_gh[2 * b]) + sc(ex.k_gh[2 * b + 1]))
        want.append(O.misbehaviour_prove(sks[accuser[b] - 1], enc[b], w[b]))
    sk_c = b"".join(sks[j - 1] for j in accuser)
    pk_c = b"".join(pks[j - 1] for j in accuser)
    E_c = b"".join(Erows[i - 1] for i in accused)
    assert chunks(be.misbehaviour_prove(sk_c, b"".join(enc), b"".join(w)), 192) == want
    assert chunks(be.complaints_prove(sk_c, b"".join(enc), b"".join(w)), 192) == want
    forged = []
    for b, p in enumerate(want):
        off = 96 if b % 2 else 160  # r1 / r2
        v = (int.from_bytes(p[off:off + 32], "little") + 1) % L
        forged.append(p[:off] + sc(v) + p[off + 32:])
    for proofs, verdict in ((want, 0), (forged, 1)):
        assert [O.complaint1_verify(h, t, accuser[b], pks[accuser[b] - 1], enc[b], Erows[accused[b] - 1], proofs[b])
                for b in range(C)] == [verdict] * C
        assert be.complaint1_verify(t, accuser, pk_c, b"".join(enc), E_c, b"".join(proofs)) == [verdict] * C
        try:
            for mode in (0, 1, 2):
                be.set_complaint_eval(mode)
                v, _ = be.complaints_verify(n, t, accuser, accused, b"".join(pks), b"".join(Erows), b"".join(enc),
                                            b"".join(proofs))
                assert v == [verdict] * C, mode
        finally:
            be.set_complaint_eval(0)


def test_complaint3_edges(be, ex, edge_ceremonies):
    """Round-4 complaints that disclose the edge shares (k_c3_check: one walk of the g comb serves both
    sides, h's comb is added): the honest values open E and A (FalseClaimedInequality, 2), e + 1 does not
    open E (FalseClaimedEquality, 3), and against another dealer's A row the complaint is valid (0)."""
    t = 2
    n, E, A, s, sp, pairs = edge_ceremonies[t]
    N = t + 1
    h = be.env_init(t, n, CK)
    row = lambda C, i: C[32 * N * i:32 * N * (i + 1)]  # noqa: E731
    accuser = [j + 1 for _, j in pairs]
    accused = [i + 1 for i, _ in pairs]
    share = [s[i * n + j] for i, j in pairs]
    rand = [sp[i * n + j] for i, j in pairs]
    A_rot = A[32 * N:] + A[:32 * N]
    try:
        for sh, Ax, verdict in ((share, A, 2), ([(k + 1) % L for k in share], A, 3), (share, A_rot, 0)):
            want = [O.complaint3_verify(h, t, accuser[c], sc(sh[c]), sc(rand[c]), row(E, accused[c] - 1),
                                        row(Ax, accused[c] - 1)) for c in range(n)]
            assert want == [verdict] * n
            assert be.complaint3_verify(t, accuser, cat(sh), cat(rand), b"".join(row(E, i - 1) for i in accused),
                                        b"".join(row(Ax, i - 1) for i in accused)) == want
            for mode in (0, 1, 2):
                be.set_complaint_eval(mode)
                assert be.complaints3_verify(n, t, accuser, accused, cat(sh), cat(rand), E, Ax)[0] == want, mode
    finally:
        be.set_complaint_eval(0)


# ---------------------------------------------------------------- decoder (k_decode)
def test_decode_edges(be, ex):
    """points_valid on the decoder's edge encodings -- p - 1 (rejected only because y = 0), p + k,
    bit 255, negated encodings, non-squares, small s -- and the valid ones through the MSM (N = 1,
    scalar 1) and through a caller-base comb."""
    edges = EV.decode_edges(invalid_fixture=ex.bad_fixture)
    encs = [e for _, e, _ in edges]
    want = [ref.decode(e) is not None for e in encs]
    assert ref.decode_why((ref.P - 1).to_bytes(32, "little")) == (None, "y = 0")
    assert list(be.points_valid(b"".join(encs))) == [int(v) for v in want]
    valid = [e for e, v in zip(encs, want) if v]
    assert len(valid) >= 50 and bytes(32) in valid
    one = sc(1)
    assert chunks(be.msm_batch(one * len(valid), b"".join(valid), len(valid), 1)) == valid
    picks = [e for c, e, _ in edges if c == "valid"]
    for x in (picks[1], picks[5], picks[20]):
        assert be.fixed_base_batch(one, base=x) == x
    for e, v in zip(encs, want):
        if not v:
            with pytest.raises(dkg_amd.DkgError) as ei:
                be.fixed_base_batch(one, base=e)
            assert ei.value.code == -2
            break


def test_undecodable_commitment_p_minus_1(be, golden):
    """A commitment row holding p - 1: the dealer reads MISSING in round 2 (no data, committee.rs:331-335)
    and REJECT in round 4 (an accusation, :549-555); the other dealers as in the fixture."""
    c = golden("ceremony_n10_t4.json")
    n, t = c["n"], c["t"]
    N = t + 1
    be.env_init(t, n, CK)
    bad, k = 6, 2
    pm1 = (ref.P - 1).to_bytes(32, "little")
    E, A = bytearray(H(c["E"])), bytearray(H(c["A"]))
    E[32 * (N * bad + k):32 * (N * bad + k) + 32] = pm1
    A[32 * (N * bad + k):32 * (N * bad + k) + 32] = pm1
    d2 = be.verify_pairs(n, t, 2, 0, n, bytes(E), H(c["s"]), H(c["s_prime"]))
    d4 = be.verify_pairs(n, t, 4, 0, n, bytes(A), H(c["s"]))
    for i in range(n):
        for j in range(n):
            honest = SELF if i == j else ACCEPT
            assert d2[i * n + j] == (honest if i != bad or i == j else MISSING), (i, j)
            assert d4[i * n + j] == (honest if i != bad or i == j else REJECT), (i, j)


# ---------------------------------------------------------------- lazy Horner (k_share_eval) and k_poly_eval
@pytest.mark.parametrize("n", [64, 65, 8200])
def test_share_eval_worst_case(be, n):
    """Every coefficient l - 1 (the largest accumulator the lazy reduction sees), t = 5..10 (every
    residue of t mod SC_LAZY_STEPS), with the dealer wave-uniform (n = 64) and per lane (n = 65);
    n = 8200 adds the largest x of the lazy path, 8191, and the first ones of the plain path."""
    top = sc(L - 1)
    for t in range(5, 11):
        be.env_init(t, n, CK)
        N = t + 1
        D = 3 if n < 100 else 1
        rows = [[L - 1] * N, [L - 1] * t + [1], [1] + [L - 1] * t][:D]
        coeffs = b"".join(cat(r) for r in rows)
        assert coeffs[:32 * N] == top * N
        _, _, s, sp = be.share_gen(coeffs, coeffs, D, n, t)
        want = cat(ref.poly_eval(r, x) for r in rows for x in range(1, n + 1))
        assert s == want and sp == want, t


def test_poly_eval_worst_case(be, ex):
    xs = [0, 1, 8191, 8192, 2**24 - 1]
    for N in (1, 2, 6, 11, 512):
        rows = [[L - 1] * N, cycle_to(ex.k_gh, N)]
        out = be.poly_eval_batch(b"".join(cat(r) for r in rows), len(rows), N, xs)
        assert out == cat(ref.poly_eval(r, x) for r in rows for x in xs), N


# ---------------------------------------------------------------- MSM workgroup sizes (k_msm)
@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 128, 129, 255, 256, 257])
def test_msm_shapes(be, ex, golden, N):
    """Around T = min(256, pow2 >= 64): B = 3 MSMs of N terms whose scalars come from the radix-16
    edge scalars (nibbles 0 and 15 in every position).  One variant with a single point throughout,
    one with (k, P), (k, -P) pairs whose partial sums pass through the identity."""
    B = 3
    pts = [H(e["P"]) for e in golden("kat_group.json")["mul"]][:B]
    negs = [ref.encode(ref.neg(ref.decode(p))) for p in pts]
    ks = [cycle_to(ex.k16[97 * b + N:], N) for b in range(B)]
    same = b"".join(pts[b] * N for b in range(B))
    scal = b"".join(cat(k) for k in ks)
    want = [bytes(O.msm(cat(ks[b]), pts[b] * N)) for b in range(B)]
    assert chunks(be.msm_batch(scal, same, B, N)) == want
    if N == 0:
        assert want == [bytes(32)] * B
        return
    total = lambda b: ref.mul(sum(ks[b]) % L, ref.decode(pts[b]))  # noqa: E731
    if N <= 65:  # the reference's opinion where it is cheap
        assert want == [ref.encode(total(b)) for b in range(B)]
    paired_k = [[ks[b][m // 2] for m in range(N)] for b in range(B)]
    paired_p = [b"".join((pts[b], negs[b])[m % 2] for m in range(N)) for b in range(B)]
    want = [bytes(O.msm(cat(paired_k[b]), paired_p[b])) for b in range(B)]
    if N % 2 == 0:
        assert want == [bytes(32)] * B
    assert chunks(be.msm_batch(b"".join(cat(k) for k in paired_k), b"".join(paired_p), B, N)) == want
