"""One party's share checks through the chunked evaluation (receivers.hip): dkg_commitment_eval,
dkg_verify_receivers and dkg_party_round2 against the fixtures and the CPU oracle, bit for bit.
be.verify_receiver (the serial walk, untouched) is a second witness."""
import ctypes

import pytest

import dkg_amd
from dkg_amd import ACCEPT, MISSING, REJECT, SELF, DkgError
from tests import oracle_lib as O
from tests.test_gpu import CEREMONIES, CK, FAULTS, H, L, dec_str

pytestmark = pytest.mark.gpu

INVALID = bytes.fromhex("edffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff7f")
IDENT = bytes(32)


@pytest.fixture(scope="module")
def be():
    b = dkg_amd.Backend(0)
    yield b
    b.close()


def columns(mat, n, js):
    """[M][n][32]: column js[m] of a [n][n][32] share matrix."""
    return b"".join(mat[32 * (i * n + j):32 * (i * n + j) + 32] for j in js for i in range(n))


def col_str(dec, n, js):
    return "".join(dec[i * n + j] for j in js for i in range(n))


# ---------------------------------------------------------------- fixtures: all n indices in one call
@pytest.mark.parametrize("name", CEREMONIES + FAULTS + ["ceremony_n64_t31.json"])
def test_fixture_columns(be, golden, name):
    c = golden(name)
    n, t = c["n"], c["t"]
    be.env_init(t, n, CK)
    js = list(range(n))
    E, A = H(c["E"]), H(c["A"])
    s, sp = columns(H(c["s"]), n, js), columns(H(c["s_prime"]), n, js)
    qual = bytes(1 if q else 0 for q in c["qualified"])
    exp2, exp4 = col_str(c["dec2"], n, js), col_str(c["dec4"], n, js)
    try:
        for chunk in (0, 1, 2, 3, t + 1, t + 6):
            be.set_receiver_chunk(chunk)
            assert dec_str(be.verify_receivers(n, t, 2, js, E, s, sp)) == exp2, chunk
            if chunk:
                assert be.last_receiver_chunk() == chunk
            d4 = dec_str(be.verify_receivers(n, t, 4, js, A, s))
            assert all(g == e for g, e in zip(d4, exp4) if e != "3"), chunk
            assert dec_str(be.verify_receivers(n, t, 4, js, A, s, None, qual)) == exp4, chunk
    finally:
        be.set_receiver_chunk(0)


# ---------------------------------------------------------------- commitment_eval against the oracle's MSM
def msm_eval(row, N, x):
    return O.msm(b"".join(pow(x, k, L).to_bytes(32, "little") for k in range(N)), row)


def test_commitment_eval_small(be, golden):
    c = golden("ceremony_n16_t7.json")
    n, t = c["n"], c["t"]
    N = t + 1
    js = [0, 5, 15, 1]
    inv = golden("kat_group.json")["invalid_encodings"]
    try:
        for rows in (H(c["E"]), H(c["A"])):
            exp = b"".join(msm_eval(rows[32 * N * i:32 * N * (i + 1)], N, j + 1) for j in js for i in range(n))
            for chunk in (0, 1, 5, 8, 64, 128):
                be.set_receiver_chunk(chunk)
                P, ok = be.commitment_eval(n, t, js, rows)
                assert P == exp and ok == b"\x01" * n, chunk
            bad = bytearray(rows)
            k = 32 * (N * 6 + 3)
            bad[k:k + 32] = H(inv[1])
            be.set_receiver_chunk(3)
            P, ok = be.commitment_eval(n, t, js, bytes(bad))
            assert ok == bytes(0 if i == 6 else 1 for i in range(n))
            for m in range(len(js)):
                for i in range(n):
                    e = 32 * (m * n + i)
                    assert P[e:e + 32] == (bytes(32) if i == 6 else exp[e:e + 32])
    finally:
        be.set_receiver_chunk(0)


def test_commitment_eval_spot(be, golden):
    sp = golden("spot_n256_t127.json")
    t = sp["t"]
    N = t + 1
    rows = b"".join(H(d["E"]) for d in sp["dealers"])
    js = [0, 1, 170, 254, 255]
    exp = b"".join(msm_eval(rows[32 * N * i:32 * N * (i + 1)], N, j + 1) for j in js for i in range(2))
    for d, drow in enumerate(sp["dealers"]):  # the fixture's own right-hand sides where they cover an index
        for pr in drow["pairs"]:
            if pr["receiver"] in js:
                e = 32 * (js.index(pr["receiver"]) * 2 + d)
                assert exp[e:e + 32].hex() == pr["rhs2"]
    try:
        for chunk in (0, 1, 5, 8, 64, 128):
            be.set_receiver_chunk(chunk)
            P, ok = be.commitment_eval(2, t, js, rows)
            assert P == exp and ok == b"\x01\x01", chunk
    finally:
        be.set_receiver_chunk(0)


# ---------------------------------------------------------------- shapes where the kernels can go wrong
def shaped_case(be, n, t, js, chunks):
    """Shares from be.share_gen with, per shape: a flipped share byte at a checked (i, j), an undecodable E
    row, an all-identity E row with honest-looking (zero) shares, SELF at i == j; expectations from
    O.verify_pairs on each column."""
    N = t + 1
    h = be.env_init(t, n, CK)
    a, b = dkg_amd.dealer_coefficients(b"\x5a" * 32, 3, 0, n, t)
    if n <= 256:
        E, A, s, sp = (bytearray(v) for v in be.share_gen(a, b, n, n, t))
    else:  # n = 4096: only the checked columns of the 512-MB share matrices are filled (the oracle's
        # polynomial evaluation; neither side reads another column)
        E, A = (bytearray(v) for v in be.share_gen(a, b, n, 1, t)[:2])
        s, sp = bytearray(32 * n * n), bytearray(32 * n * n)
        for j in set(js):
            x = (j + 1).to_bytes(32, "little")
            for i in range(n):
                k = 32 * (i * n + j)
                s[k:k + 32] = O.poly_eval(a[32 * N * i:32 * N * (i + 1)], x)
                sp[k:k + 32] = O.poly_eval(b[32 * N * i:32 * N * (i + 1)], x)
    i_flip, i_bad, i_id = (js[0] + 1) % n, (js[0] + 2) % n, (js[0] + 3) % n
    s[32 * (i_flip * n + js[0])] ^= 1
    for C in (E, A):
        C[32 * N * i_bad + 32:32 * N * i_bad + 64] = INVALID
        C[32 * N * i_id:32 * N * (i_id + 1)] = IDENT * N
    s[32 * n * i_id:32 * n * (i_id + 1)] = bytes(32 * n)
    sp[32 * n * i_id:32 * n * (i_id + 1)] = bytes(32 * n)
    E, A, s, sp = bytes(E), bytes(A), bytes(s), bytes(sp)
    exp = {}
    for rnd, C in ((2, E), (4, A)):
        cols = {}
        for j in set(js):  # rc = -1 only says that a row does not decode (MISSING / REJECT in the column)
            cols[j] = O.verify_pairs(n, t, rnd, C, h, s, sp if rnd == 2 else None, 0, n, j, j + 1)[0]
            assert cols[j][i_bad] == (SELF if i_bad == j else (MISSING if rnd == 2 else REJECT))
        exp[rnd] = b"".join(cols[j] for j in js)
    assert exp[2][i_flip] == REJECT and exp[2][i_id] == ACCEPT and SELF in exp[2]
    sc, spc = columns(s, n, js), columns(sp, n, js)
    try:
        for chunk in chunks:
            be.set_receiver_chunk(chunk)
            assert be.verify_receivers(n, t, 2, js, E, sc, spc) == exp[2], (n, t, chunk)
            assert be.verify_receivers(n, t, 4, js, A, sc) == exp[4], (n, t, chunk)
    finally:
        be.set_receiver_chunk(0)
    # second witness: the serial single-receiver call
    j = js[0]
    assert be.verify_receiver(n, t, 2, j, E, sc[:32 * n], spc[:32 * n]) == exp[2][:n]


@pytest.mark.parametrize("n,t,js,chunks", [
    (130, 64, [129, 0, 64, 129], (0, 8, 64)),      # N = 65: one past a wave and past chunks of 8 / 64
    (70, 34, [69, 3, 34, 3], (0, 8)),              # ragged dealer group, G = 5 at chunk 8
    (256, 127, [0, 1, 170, 254, 255, 1], (0, 8)),  # x = 1, 2, 171, 255, 256
])
def test_shapes(be, n, t, js, chunks):
    shaped_case(be, n, t, js, chunks)


# ---------------------------------------------------------------- both copies of k_recv_chunks / k_recv_fold
def test_field_modes(be, golden):
    """The chunk and fold kernels are compiled with both field multiplications and the runtime picks one
    per call: the product-scanning copies (dkg_ctx_set_field_mode 1) and the column-sum copies (2) give
    the bytes of the default, on the n = 10 fixture's columns (one chunk, and three chunks with a fold)
    and on a shape with a ragged dealer group and five chunks."""
    c = golden("ceremony_n10_t4.json")
    n, t = c["n"], c["t"]
    js = list(range(n))
    E, A = H(c["E"]), H(c["A"])
    s, sp = columns(H(c["s"]), n, js), columns(H(c["s_prime"]), n, js)
    qual = bytes(1 if q else 0 for q in c["qualified"])
    exp2, exp4 = col_str(c["dec2"], n, js), col_str(c["dec4"], n, js)
    points = {}
    try:
        for mode in (0, 1, 2):
            be.set_field_mode(mode)
            be.env_init(t, n, CK)
            for chunk in (0, 2):
                be.set_receiver_chunk(chunk)
                assert dec_str(be.verify_receivers(n, t, 2, js, E, s, sp)) == exp2, (mode, chunk)
                assert dec_str(be.verify_receivers(n, t, 4, js, A, s, None, qual)) == exp4, (mode, chunk)
                # the evaluated points themselves: mode 0 (first) is the default's bytes
                got = be.commitment_eval(n, t, js, E)
                assert got == points.setdefault(chunk, got), (mode, chunk)
            if mode:
                shaped_case(be, 70, 34, [69, 3, 34, 3], (8,))
    finally:
        be.set_field_mode(0)
        be.set_receiver_chunk(0)


def test_wide_index_short_polynomial(be):
    """(4096, 3): multipliers of 12-13 bits, N smaller than any useful chunk."""
    shaped_case(be, 4096, 3, [4094, 4095, 2730], (0, 2))


# ---------------------------------------------------------------- the workload's own size, once
def test_workload_size(be, golden):
    n, t = 1024, 511
    N = t + 1
    h = be.env_init(t, n, CK)
    spot = golden("spot_n1024_t511.json")
    a, b = dkg_amd.dealer_coefficients(H(spot["master_seed"]), 0, 0, n, t)
    E, A, s, sp = be.share_gen(a, b, n, n, t)
    s = bytearray(s)
    js = [1023, 682]
    for i, j in ((5, 1023), (700, 682), (1023, 682)):
        s[32 * (i * n + j) + 7] ^= 0x10
    s = bytes(s)
    sc, spc = columns(s, n, js), columns(sp, n, js)
    exp = b""
    for j in js:
        col, rc = O.verify_pairs(n, t, 2, E, h, s, sp, 0, n, j, j + 1)
        assert rc == 0
        exp += col
    assert [k for k in range(2 * n) if exp[k] == REJECT] == [5, n + 700, n + 1023]
    wit = b"".join(be.verify_receiver(n, t, 2, j, E, sc[32 * n * m:32 * n * (m + 1)], spc[32 * n * m:32 * n * (m + 1)])
                   for m, j in enumerate(js))
    assert wit == exp
    try:
        for chunk in (0, 8):
            be.set_receiver_chunk(chunk)
            assert be.verify_receivers(n, t, 2, js, E, sc, spc) == exp, chunk
            for d in spot["dealers"]:
                i = d["dealer"]
                assert E[32 * N * i:32 * N * (i + 1)].hex() == d["E"]
                P, ok = be.commitment_eval(1, t, js, H(d["E"]))
                for pr in d["pairs"]:
                    if pr["receiver"] in js:
                        m = js.index(pr["receiver"])
                        assert P[32 * m:32 * m + 32].hex() == pr["rhs2"] and ok == b"\x01"
    finally:
        be.set_receiver_chunk(0)


# ---------------------------------------------------------------- party_round2
def party_column(c, n, j):
    e1, ct = H(c["e1"]), H(c["ct"])
    k = lambda i: 64 * (i * n + j)  # noqa: E731
    return b"".join(e1[k(i):k(i) + 64] for i in range(n)), b"".join(ct[k(i):k(i) + 64] for i in range(n))


@pytest.mark.parametrize("name", ["full_n4_t1.json", "full_n10_t4.json", "full_faults_n10_t4.json"])
def test_party_round2(be, golden, name):
    c = golden(name)
    n, t = c["n"], c["t"]
    be.env_init(t, n, CK)
    s, sp, sk = H(c["s"]), H(c["s_prime"]), H(c["member_sk"])
    for j in range(n):
        e1c, ctc = party_column(c, n, j)
        r = be.party_round2(n, t, j, H(c["E"]), e1c, ctc, sk[32 * j:32 * j + 32])
        assert r["s"] == columns(s, n, [j]) and r["s_prime"] == columns(sp, n, [j])
        assert dec_str(r["dec"]) == "".join(c["dec2"][i * n + j] for i in range(n))
        assert r["complaints"] == c["complaints2"][j] and bool(r["r2_error"]) == c["r2_error"][j]
        assert r["proofs"] is None


def test_party_round2_proofs(be, golden):
    from tests.test_oracle import VERDICT, _complaint_inputs
    cp = golden("complaints_n10_t4.json")
    c = golden(cp["source"])
    n, t = c["n"], c["t"]
    h = be.env_init(t, n, CK)
    sk = H(c["member_sk"])
    seen = set()
    for x in cp["round1"]:
        j, i = x["accuser"] - 1, x["accused"] - 1
        e1c, ctc = party_column(c, n, j)
        rej = [k for k in range(n) if c["dec2"][k * n + j] == "0"]
        if i not in rej or (j, i) in seen:
            continue  # a forged complaint of the fixture: this party raises none against that dealer
        seen.add((j, i))
        w = bytearray(64 * n)
        w[64 * i:64 * i + 64] = b"".join(H(v) for v in x["w"])
        r = be.party_round2(n, t, j, H(c["E"]), e1c, ctc, sk[32 * j:32 * j + 32], bytes(w))
        _, pk, enc, Erow, proof = _complaint_inputs(cp, c, x)
        got = r["proofs"][192 * i:192 * i + 192]
        assert got == proof
        assert O.complaint1_verify(h, t, x["accuser"], pk, enc, Erow, got) == VERDICT[x["verdict"]]
        for k in range(n):
            if k not in rej:
                assert r["proofs"][192 * k:192 * k + 192] == bytes(192)
    assert seen, "the fixture lists real complaints"
    # an e1 that does not decode: missing data, no complaint and no proof
    j, i = 2, 7
    e1c, ctc = party_column(c, n, j)
    base = be.party_round2(n, t, j, H(c["E"]), e1c, ctc, sk[32 * j:32 * j + 32], bytes(64 * n))
    bad = bytearray(e1c)
    bad[64 * i + 32:64 * i + 64] = INVALID
    r = be.party_round2(n, t, j, H(c["E"]), bytes(bad), ctc, sk[32 * j:32 * j + 32], bytes(range(64)) * n)
    assert r["dec"][i] == MISSING and r["proofs"][192 * i:192 * i + 192] == bytes(192)
    assert r["complaints"] == base["complaints"] - (1 if base["dec"][i] == REJECT else 0)
    assert bytes(v for k, v in enumerate(r["dec"]) if k != i) == bytes(v for k, v in enumerate(base["dec"]) if k != i)


# ---------------------------------------------------------------- phase records
def test_phase_records(golden):
    """recv.* and pairs.* of every one-party call on one stream: which phases a call records and which read
    -1; with the default two streams every key reads -1, the records of earlier calls included."""
    c = golden("full_n10_t4.json")
    n, t = c["n"], c["t"]
    E, sk = H(c["E"]), H(c["member_sk"])
    s, sp = columns(H(c["s"]), n, [1, 3]), columns(H(c["s_prime"]), n, [1, 3])
    j, i = 1, 4
    e1c, ctc = party_column(c, n, j)
    bad = bytearray(ctc)
    bad[64 * i + 32] ^= 1  # dealer i's share to j, corrupted in transit
    w = bytes(range(64)) * n
    recv, pairs = ("decrypt", "decode", "chunks", "fold", "check", "prove"), ("decode", "eval")

    def calls(b, want_recv, want_pairs):
        """every call; want_*(ran): the phase times expected, ran = the keys the call records"""
        b.set_receiver_chunk(2)
        b.commitment_eval(n, t, [1], E)
        want_recv({"decode", "chunks", "fold"})
        b.set_receiver_chunk(t + 1)  # one chunk: the serial walk
        b.commitment_eval(n, t, [1], E)
        want_recv({"decode", "chunks"})
        b.set_receiver_chunk(0)
        b.verify_receivers(n, t, 2, [1, 3], E, s, sp)
        ph = b.phase_times("recv")
        want_recv({"decode", "chunks", "check"} | ({"fold"} if ph["fold"] >= 0 else set()))
        r = b.party_round2(n, t, j, E, e1c, bytes(bad), sk[32 * j:32 * j + 32], w)
        assert r["dec"][i] == REJECT and r["complaints"] == 1
        ph = b.phase_times("recv")
        want_recv({"decrypt", "decode", "chunks", "check", "prove"} | ({"fold"} if ph["fold"] >= 0 else set()))
        r = b.party_round2(n, t, j, E, e1c, ctc, sk[32 * j:32 * j + 32], w)
        assert r["complaints"] == 0
        ph = b.phase_times("recv")
        want_recv({"decrypt", "decode", "chunks", "check"} | ({"fold"} if ph["fold"] >= 0 else set()))
        b.commitment_eval_pairs(n, t, [0, 2, 2], [1, 1, 5], E)
        want_pairs({"decode", "eval"})

    b = dkg_amd.Backend(0)
    try:
        b.env_init(t, n, CK)

        def expect(tag, names, recorded):
            def want(ran):
                ph = b.phase_times(tag)
                for k in names:
                    assert ph[k] >= 0 if recorded and k in ran else ph[k] == -1, (k, ph)
            return want
        b.set_streams(1)
        calls(b, expect("recv", recv, True), expect("pairs", pairs, True))
        b.set_streams(2)  # the default
        calls(b, expect("recv", recv, False), expect("pairs", pairs, False))
    finally:
        b.close()


# ---------------------------------------------------------------- argument errors
def test_argument_errors(golden):
    c = golden("ceremony_n10_t4.json")
    n, t = c["n"], c["t"]
    E, s, sp = H(c["E"]), columns(H(c["s"]), n, [1]), columns(H(c["s_prime"]), n, [1])
    b = dkg_amd.Backend(0)
    try:
        with pytest.raises(DkgError) as e:  # no dkg_env_init
            b.verify_receivers(n, t, 2, [1], E, s, sp)
        assert e.value.code == -1 and "dkg_env_init" in str(e.value)
        assert b.verify_receivers(n, t, 2, [], E, b"", b"") == b""  # M = 0 touches nothing
        dec = ctypes.create_string_buffer(b"\x07" * n, n)
        arr = (ctypes.c_uint32 * 1)(1)
        assert dkg_amd.lib().dkg_verify_receivers(b._ctx, n, t, 2, 0, arr, None, None, None, None, dec) == 0
        assert dec.raw == b"\x07" * n
        b.env_init(t, n, CK)
        for rnd, js, spc in ((3, [1], sp), (2, [n], sp), (2, [1, n + 5], sp), (2, [1], None)):
            with pytest.raises(DkgError) as e:
                b.verify_receivers(n, t, rnd, js, E, s * len(js), spc)
            assert e.value.code == -1
        with pytest.raises(DkgError):
            b.commitment_eval(n, t, [1 << 24], E)
        assert b.last_receiver_chunk() == 0  # no call got as far as a plan
        assert dec_str(b.verify_receivers(n, t, 2, [1], E, s, sp)) == "".join(c["dec2"][i * n + 1] for i in range(n))
    finally:
        b.close()
