"""The two builders of the radix-2^BITS comb tables (dkg_ctx_set_comb_build): 1 = one thread per entry
(k_build_combw), 2 = chained (comb_build.hip).  Mode 1 is the yardstick: the tables' canonical contents
(dkg_comb_entries) must agree byte for byte, for whole tables of the member keys' geometry and for the
ranges of the shared bases' geometry where the chained builder's chunks begin and end; a sample of the
entries is also recomputed with the big-integer reference tests/ristretto_ref.py.  Then the consumers --
fixed-base products of a caller base, a ceremony under a commitment key of its own, full mode's
encryption -- give identical bytes under either builder, and the golden values.
"""
import random

import pytest

import dkg_amd
from dkg_amd import _lib
from tests import edge_vectors as EV
from tests import ristretto_ref as ref

pytestmark = pytest.mark.gpu

H = bytes.fromhex
P = ref.P
MODES = (1, 2)


@pytest.fixture(scope="module")
def be():
    b = dkg_amd.Backend(0)
    yield b
    b.set_comb_build(0)
    b.close()


def seeded_point(seed):
    k = random.Random(seed).randrange(1, ref.L)
    return ref.encode(ref.mul(k, ref.BASE))


def le(v):
    return (v % P).to_bytes(32, "little")


def entry_bytes(p):
    """The 96 bytes of a comb entry for the point p (extended coordinates): y+x, y-x, 2dxy of the affine
    point, canonical little-endian."""
    zi = ref.inv(p[2])
    x, y = p[0] * zi % P, p[1] * zi % P
    return le(y + x) + le(y - x) + le(2 * ref.D * x * y)


def ref_range(base, bits, window, first, count):
    """Entries d = first + 1 .. first + count of `window`: d * 2^(bits * window) * P, P the RFC 9496
    decode of `base`."""
    bw = ref.decode(base)
    assert bw is not None
    for _ in range(bits * window):
        bw = ref.double(bw)
    p = ref.mul(first + 1, bw)
    out = []
    for _ in range(count):
        out.append(entry_bytes(p))
        p = ref.add(p, bw)
    return b"".join(out)


def build_under(be, mode, kind, base, window, first, count):
    be.set_comb_build(mode)
    out = be.comb_entries(kind, base, window, first, count)
    assert be.last_comb_build() == mode
    assert len(out) == 96 * count
    return out


# ---- the member keys' geometry: whole tables
def key_bases(golden):
    return {
        "generator": None,
        "h": H(golden("ceremony_n10_t4.json")["h"]),  # the commitment key of CK_DEFAULT
        "member_pk": H(golden("full_n10_t4.json")["member_pk"])[32:64],
        "identity": bytes(32),
        "seeded": seeded_point(20261),
    }


@pytest.mark.parametrize("name", ["generator", "h", "member_pk", "identity", "seeded"])
def test_key_tables_agree_entry_for_entry(be, golden, name):
    g = dkg_amd.comb_geometry(1)
    base = key_bases(golden)[name]
    if name == "h":
        assert base == be.env_init(4, 10)
    for w in range(g["windows"]):
        one = build_under(be, 1, 1, base, w, 0, g["entries"])
        two = build_under(be, 2, 1, base, w, 0, g["entries"])
        assert one == two, (name, w)
        if name == "identity":
            assert two == (le(1) + le(1) + le(0)) * g["entries"], w
    # the two ends of the table against the big-integer reference
    enc = ref.BASE_BYTES if base is None else base
    top = g["windows"] - 1
    assert build_under(be, 2, 1, base, 0, 0, 3) == ref_range(enc, g["bits"], 0, 0, 3)
    assert build_under(be, 2, 1, base, top, g["entries"] - 2, 2) == ref_range(enc, g["bits"], top, g["entries"] - 2, 2)


# ---- the shared bases' geometry: the ranges around the chunk boundaries
def shared_ranges():
    g = dkg_amd.comb_geometry(0)
    S, E, W = g["chunk"], g["entries"], g["windows"]
    mid = W // 2
    rs = [(0, 0, 2 * S + 2)]                                   # window 0, entries 1 .. 2S+2
    for k in (1, E // (2 * S), E // S - 1):                    # entries kS-1 .. kS+2; the last chunk included
        rs.append((mid, k * S - 2, 4))
    rs.append((W - 1, E - S - 1, S + 1))                       # the top window's last S+1 entries
    # whole chunks away from the ends, for the reference sample (about 200 entries in all)
    rs.append((1, 37 * S, 64 + 2 * S))
    rs.append((W - 2, E // 2 - 3 * S - 1, 84 + 2 * S))
    rs.append((W - 1, 0, S + 2))
    return g, rs


def test_shared_ranges_agree_and_match_the_reference(be):
    g, rs = shared_ranges()
    base = seeded_point(20262)
    # entry (0, 1) under the yardstick first: the base itself, so a disagreement between the two decoders
    # shows up here and not as a builder bug
    first = build_under(be, 1, 0, base, 0, 0, 1)
    assert first == entry_bytes(ref.decode(base))
    checked = 0
    for w, f, c in rs:
        one = build_under(be, 1, 0, base, w, f, c)
        two = build_under(be, 2, 0, base, w, f, c)
        assert one == two, (w, f, c)
        assert two == ref_range(base, g["bits"], w, f, c), (w, f, c)
        checked += c
    assert checked >= 180
    assert be.last_comb_build_ms() > 0


def test_generator_table_ends(be):
    """base = NULL is the generator: the first and the last entry of the shared geometry."""
    g = dkg_amd.comb_geometry(0)
    W, E = g["windows"], g["entries"]
    for mode in MODES:
        assert build_under(be, mode, 0, None, 0, 0, 2) == ref_range(ref.BASE_BYTES, g["bits"], 0, 0, 2)
        assert build_under(be, mode, 0, None, W - 1, E - 1, 1) == ref_range(ref.BASE_BYTES, g["bits"], W - 1, E - 1, 1)


# ---- through the consumers
def test_fixed_base_on_a_caller_base(be):
    """dkg_fixed_base_batch with a caller's base: every window's edge digits (0, +-1, +-2^(bits-1), the
    carries) under both builders."""
    B = dkg_amd.comb_geometry(0)["bits"]
    ks = EV.comb_scalars(B)
    assert {0, 1, ref.L - 1} <= set(ks)
    base = seeded_point(20263)
    scalars = b"".join(ref.sc(k) for k in ks)
    out = {}
    for mode in MODES:
        be.set_comb_build(mode)
        out[mode] = be.fixed_base_batch(scalars, base)
        assert be.last_comb_build() == mode
    assert out[1] == out[2]
    tab = ref.doublings(ref.decode(base))
    for k in (0, 1, ref.L - 1, ks[0], ks[len(ks) // 2]):
        i = ks.index(k)
        assert out[2][32 * i:32 * i + 32] == ref.encode(ref.mul_doublings(k, tab)), k


def check_ceremony(c, r):
    dec = lambda d: "".join(str(x) for x in d)  # noqa: E731
    assert r.E.hex() == c["E"] and r.A.hex() == c["A"]
    assert r.s.hex() == c["s"] and r.s_prime.hex() == c["s_prime"]
    assert dec(r.dec2) == c["dec2"] and dec(r.dec4) == c["dec4"]
    assert r.qualified == c["qualified"] and r.reconstruct == c["reconstruct"]
    assert r.final_share.hex() == c["final_share"] and r.public_share.hex() == c["public_share"]
    assert r.mpk.hex() == c["mpk"]


def test_ceremony_under_a_commitment_key_of_its_own(be, golden):
    """dkg_env_init builds h's comb with the ctx's builder; the n = 8 golden ceremony under that key."""
    c = golden("ceremony_n8_t3_ck.json")
    n, t = c["n"], c["t"]
    ck = H(c["ck_bytes"])
    assert (n, t) == (8, 3) and ck != dkg_amd.api.CK_DEFAULT
    a, b = H(c["a"]), H(c["b"])
    res = {}
    for mode in MODES:
        be.set_comb_build(mode)
        assert be.env_init(t, n, ck).hex() == c["h"]
        assert be.last_comb_build() == mode and be.last_comb_build_ms() > 0
        res[mode] = be.ceremony(a, b, n, t)
        check_ceremony(c, res[mode])
    for f in ("E", "A", "s", "s_prime", "dec2", "dec4", "final_share", "public_share", "mpk"):
        assert getattr(res[1], f) == getattr(res[2], f), f


def test_full_mode_encryption_on_radix_2_10_key_combs(be, golden):
    """dkg_encrypt_shares / dkg_decrypt_shares at n = 8 with the radix-2^DKG_KEY_COMB_BITS key combs
    forced: the golden wire ciphertexts under either builder."""
    c = golden("full_n8_t3.json")
    n = c["n"]
    assert n == 8
    sk, pk = H(c["member_sk"]), H(c["member_pk"])
    s, sp, r = H(c["s"]), H(c["s_prime"]), H(c["enc_r"])
    be.env_init(c["t"], n)
    be.set_key_comb(1)
    try:
        out = {}
        for mode in MODES:
            be.set_comb_build(mode)  # drops the cached key combs: the encryption below rebuilds them
            out[mode] = be.encrypt_shares(pk, s, sp, r, n, n)
            assert be.last_key_comb() == 1 and be.last_comb_build() == mode
            assert out[mode][0].hex() == c["e1"] and out[mode][1].hex() == c["ct"]
            ds, dsp, ok = be.decrypt_shares(sk, out[mode][0], out[mode][1], n, n)
            assert ds == s and dsp == sp and set(ok) == {1}
        assert out[1] == out[2]
    finally:
        be.set_key_comb(0)


# ---- bookkeeping
def test_bookkeeping_follows_the_setter(be):
    base = seeded_point(20264)
    one = ref.sc(1)
    be.set_comb_build(1)
    assert be.fixed_base_batch(one, base) == base
    assert be.last_comb_build() == 1
    ms1 = be.last_comb_build_ms()
    assert ms1 > 0
    # the same base again: its comb is cached, nothing is built ...
    assert be.fixed_base_batch(one, base) == base
    assert be.last_comb_build_ms() == ms1
    # ... until the setter drops it: the next call builds with the new builder
    be.set_comb_build(2)
    assert be.fixed_base_batch(one, base) == base
    assert be.last_comb_build() == 2
    assert be.last_comb_build_ms() > 0
    # automatic resolves to one of the two builders
    be.set_comb_build(0)
    assert be.fixed_base_batch(one, base) == base
    assert be.last_comb_build() in MODES


def test_a_fresh_context_has_built_the_generator_comb():
    b = dkg_amd.Backend(0)
    try:
        assert b.last_comb_build() in MODES and b.last_comb_build_ms() > 0
        for mode in (-1, 3):
            with pytest.raises(dkg_amd.DkgError) as e:
                b.set_comb_build(mode)
            assert e.value.code == _lib.DKG_E_ARG
    finally:
        b.close()


# ---- argument errors of dkg_comb_entries
def test_comb_entries_argument_errors(be, golden):
    bad = H(golden("kat_group.json")["invalid_encodings"][0])
    be.set_comb_build(2)
    for kind in (0, 1):
        g = dkg_amd.comb_geometry(kind)
        W, E = g["windows"], g["entries"]
        for args in [(-1, 0, 1), (W, 0, 1), (0, E, 1), (0, E - 1, 2), (0, 0, E + 1), (0, E + 1, 0)]:
            with pytest.raises(dkg_amd.DkgError) as e:
                be.comb_entries(kind, None, *args)
            assert e.value.code == _lib.DKG_E_ARG, (kind, args)
        with pytest.raises(dkg_amd.DkgError) as e:
            be.comb_entries(kind, bad, 0, 0, 1)
        assert e.value.code == _lib.DKG_E_DECODE
        # count == 0 touches nothing: not the base (which does not decode), not the output
        assert be.comb_entries(kind, bad, 0, 0, 0) == b""
        assert be.comb_entries(kind, None, W - 1, E, 0) == b""
        assert _lib.lib().dkg_comb_entries(be._ctx, kind, None, 0, 0, 0, None) == _lib.DKG_OK
    for kind in (-1, 2):
        with pytest.raises(dkg_amd.DkgError) as e:
            be.comb_entries(kind, None, 0, 0, 1)
        assert e.value.code == _lib.DKG_E_ARG
