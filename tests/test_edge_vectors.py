"""CPU checks of the big-integer reference (tests/ristretto_ref.py) and of the edge vectors
(tests/edge_vectors.py) that tests/test_gpu_edges.py feeds to the kernels.

The reference must reproduce the libsodium fixtures; the vectors must really contain the rare
recoding cases (conditions on the inputs, so the GPU tests cannot pass by leaving cases out); and
the C oracle must agree with the reference on every vector, so the GPU tests may use the oracle
where they need Blake2b or ChaCha20.
"""
import pytest

import dkg_amd
from tests import edge_vectors as EV
from tests import oracle_lib as O
from tests import ristretto_ref as ref

H = bytes.fromhex
L = ref.L


def _sc(hexstr):
    return ref.from_bits(H(hexstr))


# ---- the reference against the libsodium fixtures
def test_ref_base_multiples_and_base_mul(golden):
    g = golden("kat_group.json")
    assert ref.BASE_BYTES == H("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76")
    assert ref.encode(ref.IDENTITY) == bytes(32)
    for e in g["base_multiples"]:
        assert ref.encode(ref.mul(e["k"], ref.BASE)).hex() == e["P"], e["k"]
    tab = ref.doublings(ref.BASE)
    for e in g["base_mul"]:
        assert ref.encode(ref.mul(_sc(e["k"]), ref.BASE)).hex() == e["P"]
        assert ref.encode(ref.mul_doublings(_sc(e["k"]), tab)).hex() == e["P"]


def test_ref_mul_add_msm(golden):
    g = golden("kat_group.json")
    for e in g["mul"]:
        p = ref.decode(H(e["P"]))
        assert p is not None and ref.encode(p).hex() == e["P"]
        assert ref.encode(ref.mul(_sc(e["k"]), p)).hex() == e["kP"]
    for e in g["add"]:
        p, q = ref.decode(H(e["P"])), ref.decode(H(e["Q"]))
        assert ref.encode(ref.add(p, q)).hex() == e["sum"]
        assert ref.encode(ref.add(p, ref.neg(q))).hex() == e["diff"]
        assert ref.encode(ref.neg(p)).hex() == e["neg_P"]
        assert ref.equals(ref.add(p, q), ref.decode(H(e["sum"]))) and not ref.equals(p, q)
        assert ref.encode(ref.double(p)) == ref.encode(ref.add(p, p))
    for c in g["msm"]:
        N = c["N"]
        sc, pt = H(c["scalars"]), H(c["points"])
        ks = [ref.from_bits(sc[32 * i:32 * i + 32]) for i in range(N)]
        ps = [ref.decode(pt[32 * i:32 * i + 32]) for i in range(N)]
        assert ref.encode(ref.msm(ks, ps)).hex() == c["out"], N


def test_ref_invalid_encodings(golden):
    for x in golden("kat_group.json")["invalid_encodings"]:
        assert ref.decode(H(x)) is None, x


def test_ref_scalars(golden):
    s = golden("kat_scalar.json")
    for e in s["ops"]:
        a, b = _sc(e["a"]), _sc(e["b"])
        assert ref.sc(a + b).hex() == e["add"] and ref.sc(a - b).hex() == e["sub"]
        assert ref.sc(a * b).hex() == e["mul"] and ref.sc(-a).hex() == e["neg_a"]
        assert ref.sc(pow(a, L - 2, L)).hex() == e["inv_a"]
    kt = s["poly_tests"]
    assert ref.poly_eval(kt["coeffs"], kt["x"]) == kt["value"]
    for e in s["poly_eval"]:
        c = H(e["coeffs"])
        coeffs = [ref.from_bits(c[32 * i:32 * i + 32]) for i in range(len(c) // 32)]
        assert [ref.sc(ref.poly_eval(coeffs, x)).hex() for x in e["points"]] == e["values"]
    assert ref.from_bits(b"\xff" * 32) == (2**255 - 1) % L  # bit 255 dropped, groups.rs:29-36
    assert ref.from_bits(ref.sc(5)[:31] + b"\x80") == 5


# ---- coverage conditions on the comb vectors
def radices():
    lib = dkg_amd.lib()
    return sorted({EV.comb_radix(lib.dkg_fixed_base_windows()), EV.comb_radix(lib.dkg_key_comb_windows()), 4})


def test_radices_are_the_documented_ones():
    assert radices() == [4, 10, 19]


@pytest.mark.parametrize("B", [4, 10, 19])
def test_comb_scalars_cover_every_window(B):
    assert B in radices()
    ks = EV.comb_scalars(B)
    assert len(ks) == {19: 184, 10: 352, 4: 884}[B]
    assert all(0 <= k < L for k in ks)
    E, W, low = 1 << (B - 1), EV.comb_windows(B), EV.comb_low_windows(B)
    seen = [set() for _ in range(W)]
    carried = [False] * W
    for k in ks:
        digits, carries = EV.comb_recode(k, B)
        assert all(-E <= d < E for d in digits)
        for w in range(W):
            seen[w].add(digits[w])
            carried[w] = carried[w] or carries[w] == 1
    for w in range(low):
        assert {-E, -1, 0, 1, E - 1} <= seen[w], (B, w)
        # with a carry in as well as without: the values either side of each edge
        assert {-E + 1, -2} <= seen[w] and (w == 0 or {-E + 2, 2} <= seen[w]), (B, w)
    # every window carries into the next, the top window included: the one that holds bit 252 (the
    # last of a comb whose radix does not divide 256; the 64th of the radix-16 comb); it never carries out
    top = 252 // B
    assert top == low and top in (W - 1, W - 2)
    assert all(carried[:top]) and not any(carried[top:]), (B, carried)
    assert {0, 1} <= seen[top] and (top == W - 1 or seen[W - 1] == {0})


def test_naf_scalars_cover_the_window_chains():
    ks = EV.naf_scalars()
    assert 35 <= len(ks) <= 48 and len(set(ks)) == len(ks) and all(0 <= k < L for k in ks)
    for k in (0, 1, 2, 3, 2**252, 2**252 - 1, L - 1, 2**64 - 1, 2**251):
        assert k in ks
    for k in ks:
        for rec in (EV.naf(k), EV.wnaf4(k)):
            assert sum(d << i for i, d in enumerate(rec)) == k
    w4 = [EV.wnaf4(k) for k in ks]
    for rec in w4:
        nz = [i for i, d in enumerate(rec) if d]
        assert all(d % 2 and abs(d) <= 7 for d in rec if d) and all(b - a >= 4 for a, b in zip(nz, nz[1:]))
        assert len(rec) <= 254 and len(nz) <= 64
    # 64 nonzero digits is the most a scalar below l can hold: bits 0, 4, .., 252
    assert max(sum(1 for d in rec if d) for rec in w4) == 64
    assert any(len(rec) == 253 and sum(1 for d in rec if d) == 1 for rec in w4)  # 2^252
    # bitwise NAF: a carry run through every bit (2^252 - 1 -> 2^252 - 1), and the densest form
    assert any(len(EV.naf(k)) == 253 and sum(1 for d in EV.naf(k) if d) == 2 for k in ks)
    assert max(sum(1 for d in EV.naf(k) if d) for k in ks) >= 126


# ---- the oracle agrees with the reference on every vector
def test_oracle_agrees_with_reference_on_edge_scalars(golden):
    ks = EV.comb_scalars(19) + EV.comb_scalars(10) + EV.comb_scalars(4) + EV.naf_scalars()
    tab = ref.doublings(ref.BASE)
    for k in ks:
        assert O.base_mul(ref.sc(k)) == ref.encode(ref.mul_doublings(k, tab)), hex(k)
    # msm: runs of 8 consecutive vectors against 8 fixture points
    enc = [H(e["P"]) for e in golden("kat_group.json")["mul"]][:8]
    tabs = [ref.doublings(ref.decode(x)) for x in enc]
    for i in range(0, len(ks), 8):
        run = ks[i:i + 8]
        want = ref.IDENTITY
        for k, t in zip(run, tabs):
            want = ref.add(want, ref.mul_doublings(k, t))
        got = O.msm(b"".join(ref.sc(k) for k in run), b"".join(enc[:len(run)]))
        assert got == ref.encode(want), i


# ---- the decoder's edge encodings
def test_decode_edges_partition(golden):
    fixture = [H(x) for x in golden("kat_group.json")["invalid_encodings"]]
    edges = EV.decode_edges(invalid_fixture=fixture)
    classes = {}
    for cls, enc, expected in edges:
        assert len(enc) == 32
        p, why = ref.decode_why(enc)
        if expected is not None:
            assert (p is not None) == expected, (cls, enc.hex(), why)
        if p is not None:
            assert ref.encode(p) == enc  # a valid encoding is the canonical one of its point
        classes.setdefault(cls, []).append(why)
    assert classes["p-1"] == ["y = 0"]  # even, canonical, square, t = 0: only the y test rejects it
    assert set(classes["non-canonical"]) == {"non-canonical"} and len(classes["non-canonical"]) == 19
    assert set(classes["bit255"]) == {"non-canonical"}
    assert set(classes["negated"]) == {"negative s"} and set(classes["negative-s"]) == {"negative s"}
    assert classes["not square"] == ["not square"] * 8 and classes["negative t"] == ["negative t"] * 8
    assert len(classes["valid"]) == 50 and len(classes["fixture"]) == 16
    assert classes["small-even"][0] is None  # s = 0 is the identity
    assert any(w is None for w in classes["small-even"][1:]) and any(w for w in classes["small-even"])
    # the 29 bad encodings of RFC 9496 appendix A.3 fall into these five reasons, all present here
    reasons = {w for ws in classes.values() for w in ws if w}
    assert reasons == {"non-canonical", "negative s", "not square", "negative t", "y = 0"}
    # the oracle's decoder agrees on every edge
    for cls, enc, _ in edges:
        assert (O.lib().or_pt_valid(enc) == 1) == (ref.decode(enc) is not None), (cls, enc.hex())


def test_share_at_hits_the_share():
    import random

    rng = random.Random(5)
    pool = EV.comb_scalars(19)
    for e in (0, 1, L - 1, pool[17]):
        for t in (0, 2, 5):
            for x in (1, 7, 190):
                c = EV.share_at(e, x, t, rng)
                assert len(c) == t + 1 and ref.poly_eval(c, x) == e
                c = EV.share_at(e, x, t, rng, pool=pool)
                assert ref.poly_eval(c, x) == e and all(a in pool for a in c[1:])
