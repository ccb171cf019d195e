#!/usr/bin/env python3
"""Generate the golden fixtures in tests/golden/ (container-only; needs libsodium 1.0.18).

This is an independent restatement of the reference's plaintext-mode ceremony
(/root/reference/src/dkg/committee.rs rounds 1-5, src/polynomial.rs, src/groups.rs) written on
libsodium's ristretto255 (RFC 9496) and Python big-int arithmetic mod l.  It shares no code with
the C oracle (oracle/) or the HIP path (dkg_amd/csrc/), so agreement of all three pins parity.
libsodium is NOT shipped and is never loaded by tests, smoke() or bench.py: only the JSON files it
writes travel.

Run:  python tools/gen_golden.py            (about a minute)
"""
import ctypes
import hashlib
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import r255  # noqa: E402  (pure-Python RFC 9496 restatement, used as a second cross-check)

L = r255.L
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
SO = ctypes.CDLL("/opt/conda/lib/libsodium.so")
assert SO.sodium_init() >= 0

CK_BYTES = b"Example of a shared string."  # every reference test (committee.rs:1079 ...)


def hx(b):
    return b.hex()


def buf(n):
    return ctypes.create_string_buffer(n)


# ---------------- group via libsodium (identity = 32 zero bytes) ----------------
ID = bytes(32)


def scb(x):
    return (x % L).to_bytes(32, "little")


def gmul_base(k):
    k %= L
    if k == 0:
        return ID
    o = buf(32)
    SO.crypto_scalarmult_ristretto255_base(o, scb(k))
    return o.raw


def gmul(p, k):
    k %= L
    if k == 0 or p == ID:
        return ID
    o = buf(32)
    SO.crypto_scalarmult_ristretto255(o, scb(k), p)  # rc = -1 only for an identity result
    return o.raw


def gadd(p, q):
    if p == ID:
        return q
    if q == ID:
        return p
    o = buf(32)
    assert SO.crypto_core_ristretto255_add(o, p, q) == 0
    return o.raw


def gneg(p):
    return gmul(p, L - 1)


def hash_to_group(msg):
    h = hashlib.blake2b(msg, digest_size=64).digest()
    o = buf(32)
    SO.crypto_core_ristretto255_from_hash(o, h)
    return o.raw


def valid(p):
    return SO.crypto_core_ristretto255_is_valid_point(p) == 1 or p == ID


def msm(scalars, points):
    acc = ID
    for s, p in zip(scalars, points):
        acc = gadd(acc, gmul(p, s))
    return acc


# ---------------- RNG (rand_chacha ChaCha20Rng == IETF ChaCha20, zero nonce) ----------------
def chacha_stream(key, nbytes):
    o = buf(nbytes)
    SO.crypto_stream_chacha20_ietf(o, ctypes.c_ulonglong(nbytes), bytes(12), key)
    return o.raw


def wide_reduce(b64):
    o = buf(32)
    SO.crypto_core_ristretto255_scalar_reduce(o, b64)
    assert o.raw == scb(int.from_bytes(b64, "little"))
    return int.from_bytes(o.raw, "little")


def dealer_seed(master, ceremony, dealer):
    return hashlib.blake2b(b"dkg-amd/v1/dealer" + master + ceremony.to_bytes(4, "little")
                           + dealer.to_bytes(4, "little"), digest_size=32).digest()


def dealer_coeffs(seed, t):
    """committee.rs:143-146: hiding polynomial (b) drawn first, then sharing polynomial (a)."""
    st = chacha_stream(seed, 2 * (t + 1) * 64)
    b = [wide_reduce(st[64 * k:64 * k + 64]) for k in range(t + 1)]
    a = [wide_reduce(st[64 * (t + 1 + k):64 * (t + 2 + k)]) for k in range(t + 1)]
    return a, b


def evaluate(coeffs, x):
    """polynomial.rs:68-74 power-sum."""
    acc, xp = 0, 1
    for c in coeffs:
        acc = (acc + c * xp) % L
        xp = xp * x % L
    return acc


def lagrange_at_zero(ys, xs):
    """polynomial.rs:162-184 at evaluation point 0."""
    res = 0
    for xa, ya in zip(xs, ys):
        coef = 1
        for xb in xs:
            if xb != xa:
                coef = coef * (0 - xb) * pow(xa - xb, -1, L) % L
        res = (res + coef * ya) % L
    return res


# ---------------- the ceremony (plaintext-share mode) ----------------
def ceremony(n, t, master, ceremony_id=0, faults=None, with_coeffs=True, transport=None, ck=CK_BYTES):
    """Returns a dict of inputs/outputs.  faults: list of dicts
       {"kind": "E_identity", "dealer": i} (committee.rs:1127-1128 style),
       {"kind": "share_flip", "dealer": i, "receiver": j}   s_ij += 1,
       {"kind": "rand_flip", "dealer": i, "receiver": j}    s'_ij += 1,
       {"kind": "A_generator", "dealer": i}                  round-3 broadcast := [g; t+1] (:1303-1306),
       {"kind": "self_share_flip", "dealer": i}              s_ii += 1 (the dealer's share to itself,
                                                             never checked: the diagonal is "self").
       Dealers / receivers are 1-based as in the reference."""
    faults = faults or []
    assert t < (n + 1) // 2, "Environment::init asserts threshold < (nr_members + 1) / 2"
    h = hash_to_group(ck)
    g = gmul_base(1)
    A, B, E, Apub, S, SP = [], [], [], [], [], []
    for i in range(n):
        a, b = dealer_coeffs(dealer_seed(master, ceremony_id, i), t)
        A.append(a)
        B.append(b)
        ap = [gmul_base(ak) for ak in a]                                # committee.rs:155
        E.append([gadd(gmul(h, bk), apk) for bk, apk in zip(b, ap)])  # committee.rs:156
        Apub.append(ap)
        S.append([evaluate(a, j + 1) for j in range(n)])                # committee.rs:165-167
        SP.append([evaluate(b, j + 1) for j in range(n)])
    # wire values after fault injection
    Ew = [list(e) for e in E]
    Aw = [list(x) for x in Apub]
    Sw = [list(s) for s in S]
    SPw = [list(s) for s in SP]
    extra = {}
    if transport is not None:  # full mode: shares travel hybrid-encrypted (committee.rs:169-172, 282-286)
        Sw, SPw, extra = transport(S, SP)
    for f in faults:
        i = f["dealer"] - 1
        if f["kind"] == "E_identity":
            Ew[i] = [ID] * (t + 1)
        elif f["kind"] == "share_flip":
            Sw[i][f["receiver"] - 1] = (Sw[i][f["receiver"] - 1] + 1) % L
        elif f["kind"] == "rand_flip":
            SPw[i][f["receiver"] - 1] = (SPw[i][f["receiver"] - 1] + 1) % L
        elif f["kind"] == "A_generator":
            Aw[i] = [g] * (t + 1)
        elif f["kind"] == "self_share_flip":
            Sw[i][i] = (Sw[i][i] + 1) % L
        else:
            raise ValueError(f)
    # round 2 (committee.rs:273-338): decision[i][j] = receiver j accepts dealer i
    dec2 = [[2] * n for _ in range(n)]
    for j in range(n):
        pw = [pow(j + 1, k, L) for k in range(t + 1)]                  # :287-290
        for i in range(n):
            if i == j:
                continue
            lhs = gadd(gmul(h, SPw[i][j]), gmul_base(Sw[i][j]))        # :292-294
            rhs = msm(pw, Ew[i])                                       # :295-296
            dec2[i][j] = int(lhs == rhs)                               # :305
    complaints2 = [sum(1 for i in range(n) if i != j and dec2[i][j] == 0) for j in range(n)]
    r2_error = [c > t for c in complaints2]                             # :340-347
    # round 3: a valid complaint disqualifies the accused everywhere (committee.rs:370-398)
    qualified = [int(all(dec2[i][j] != 0 for j in range(n))) for i in range(n)]
    final_share = [sum(Sw[i][j] for i in range(n) if qualified[i]) % L for j in range(n)]  # :454-462
    public_share = [gmul_base(s) for s in final_share]                 # :464-466
    # round 4 (committee.rs:520-559)
    dec4 = [[2] * n for _ in range(n)]
    for j in range(n):
        pw = [pow(j + 1, k, L) for k in range(t + 1)]
        for i in range(n):
            if i == j:
                continue
            if not qualified[i]:
                dec4[i][j] = 3  # not checked: disqualified dealer is skipped (:522)
                continue
            lhs = gmul_base(Sw[i][j])                                  # :537
            rhs = msm(pw, Aw[i])                                       # :538-539
            dec4[i][j] = int(lhs == rhs)                               # :541
    # fewer than t+1 honest dealers (self included) in receiver j's round 4 (committee.rs:515-516, 567-569)
    r4_error = [1 + sum(1 for i in range(n) if i != j and qualified[i] and dec4[i][j] == 1) < t + 1
                for j in range(n)]
    # round 5 / finalise (committee.rs:625-805): accused-and-valid dealers are reconstructed
    recon = [int(qualified[i] and any(dec4[i][j] == 0 for j in range(n) if j != i)) for i in range(n)]
    # Phases<Phase4>::proceed (committee.rs:673-677): too few honest (qualified, not reconstructed)
    phase4_error = sum(qualified) - sum(recon) <= t
    final = [int(qualified[i] and not recon[i]) for i in range(n)]              # :733-739
    mpk = None
    # the disclosures a finalising final party holds: its own share plus the phase-5 broadcasts of
    # the other final parties -- which only parties that reached Phases<Phase4>::proceed send: a party
    # whose Phase1 or Phase3 proceed failed (r2 / r4 error, :340-347, 567-569, 684) never does, and
    # does not finalise itself.  So every finalising party interpolates over exactly `disc`.
    disc = [j for j in range(n) if final[j] and not r2_error[j] and not r4_error[j]]
    if not phase4_error and any(recon) and len(disc) < t:
        phase4_error_mpk = True  # InsufficientSharesForRecovery(i) for every finalising party (:779-781)
    else:
        phase4_error_mpk = phase4_error
    if not phase4_error_mpk:  # else nobody finalises: there is no master public key
        mpk = ID
        exact = True
        for i in range(n):
            if recon[i]:
                xs = [j + 1 for j in disc]
                ys = [Sw[i][x - 1] for x in xs]
                secret = lagrange_at_zero(ys, xs)                                 # :784-788
                # t points (fewer than t+1) interpolate a wrong secret, as the reference computes it
                exact &= len(xs) >= t + 1
                assert secret == A[i][0] or len(xs) < t + 1
                mpk = gadd(mpk, gmul_base(secret))                                # :789
            elif qualified[i]:
                mpk = gadd(mpk, Aw[i][0])                                         # :790-795
        # property of the honest run (committee.rs:1633-1647): mpk == g * sum of qualified secrets
        assert mpk == gmul_base(sum(A[i][0] for i in range(n) if qualified[i])) or not exact
    out = {
        "n": n, "t": t, "ceremony": ceremony_id, "master_seed": hx(master), "ck_bytes": hx(ck),
        "h": hx(h), "faults": faults,
        "E": "".join(hx(p) for e in Ew for p in e),
        "A": "".join(hx(p) for e in Aw for p in e),
        "s": "".join(hx(scb(x)) for row in Sw for x in row),
        "s_prime": "".join(hx(scb(x)) for row in SPw for x in row),
        "dec2": "".join(str(d) for row in dec2 for d in row),
        "dec4": "".join(str(d) for row in dec4 for d in row),
        "complaints2": complaints2, "r2_error": r2_error, "r4_error": r4_error, "phase4_error": phase4_error,
        "qualified": qualified,
        "reconstruct": recon,
        "final_share": "".join(hx(scb(x)) for x in final_share),
        "public_share": "".join(hx(p) for p in public_share),
        "mpk": hx(mpk) if mpk is not None else hx(ID),  # all zero: no mpk when phase4_error
    }
    out.update(extra)
    if with_coeffs:
        out["a"] = "".join(hx(scb(x)) for row in A for x in row)
        out["b"] = "".join(hx(scb(x)) for row in B for x in row)
        out["dealer_seeds"] = [hx(dealer_seed(master, ceremony_id, i)) for i in range(n)]
    out["_state"] = {"Sw": Sw, "Aw": Aw, "Apub": Apub, "qualified": qualified, "recon": recon,
                     "r2_error": r2_error, "r4_error": r4_error}
    return out


def finalise_party(p, n, t, st, disclosed, r2_error=None, r4_error=None):
    """Phases<Phase5>::finalise (committee.rs:726-805) as party p (0-based) runs it, after its own
    Phase1 / Phase3 / Phase4 proceed (a failure there stops it): (status, index, mpk).
    disclosed[q] = 0: party q's phase-5 broadcast is not fetched (MembersFetchedState5 drops None,
    :1000-1022, and never includes the party's own, :1009-1010)."""
    q, rec = st["qualified"], st["recon"]
    if r2_error and r2_error[p]:
        return "R2_ERROR", -1, None                           # :340-347
    if r4_error and r4_error[p]:
        return "R4_ERROR", -1, None                           # :567-569
    if sum(q) - sum(rec) <= t:
        return "PHASE4_ERROR", -1, None                       # :673-677
    final = [x ^ y for x, y in zip(q, rec)]                   # :733-739
    mk = ID
    for i in range(n):
        if rec[i] and q[i]:
            xs, ys = [p + 1], [st["Sw"][i][p]]                # own index and share (:754-761)
            for s_ in range(n):
                # :763-775; a party whose Phase1/Phase3 proceed failed never broadcasts phase 5
                if (s_ != p and disclosed[s_] and final[s_] and not (r2_error and r2_error[s_])
                        and not (r4_error and r4_error[s_])):
                    xs.append(s_ + 1)
                    ys.append(st["Sw"][i][s_])
            if len(xs) < t:                                   # :779-781 (threshold, not t + 1)
                return "INSUFFICIENT", i, None
            mk = gadd(mk, gmul_base(lagrange_at_zero(ys, xs)))  # :784-789
        else:
            # committed_shares[i]: set for itself at init (:190) and for qualified dealers in
            # Phase3::proceed (:527-530); expect() panics otherwise (:791-794)
            if i == p:
                mk = gadd(mk, st["Apub"][i][0])
            elif q[i]:
                mk = gadd(mk, st["Aw"][i][0])
            else:
                return "PANIC", i, None
    return "OK", -1, mk


def finalise_golden(c, cases):
    """Per-party finalise outcomes of ceremony `c` under the given disclosure / earlier-error cases."""
    n, t, st = c["n"], c["t"], c["_state"]
    out = []
    for case in cases:
        disclosed = case.get("disclosed", [1] * n)
        res = [finalise_party(p, n, t, st, disclosed, case.get("r2_error"), case.get("r4_error")) for p in range(n)]
        out.append(dict(case, status=[r[0] for r in res], index=[r[1] for r in res],
                        mpk=[hx(r[2]) if r[2] is not None else hx(ID) for r in res]))
    return out


# ---------------- full (encrypted-share) mode: elgamal.rs hybrid encryption ----------------
def member_seed(master, ceremony, member):
    return hashlib.blake2b(b"dkg-amd/v1/member" + master + ceremony.to_bytes(4, "little")
                           + member.to_bytes(4, "little"), digest_size=32).digest()


def member_keys(master, ceremony_id, n):
    """MemberCommunicationKey::new per member (procedure_keys.rs:72-76) from the seeded convention,
    returned SORTED by public-key bytes (procedure_keys.rs:26-40 Ord; committee.rs:134-135): the
    party of index q+1 is the q-th smallest key."""
    sks = [wide_reduce(chacha_stream(member_seed(master, ceremony_id, j), 64)) for j in range(n)]
    pks = [gmul_base(sk) for sk in sks]
    order = sorted(range(n), key=lambda j: pks[j])
    return [sks[j] for j in order], [pks[j] for j in order]


def enc_randomness(seed, t, n):
    """Scalar::random draws after the two polynomials (committee.rs:171-172, elgamal.rs:137):
    recipient q takes block 2(t+1) + 2q for the randomness ciphertext, the next for the share."""
    N = t + 1
    st = chacha_stream(seed, (2 * N + 2 * n) * 64)
    return [[wide_reduce(st[64 * (2 * N + 2 * q + w):64 * (2 * N + 2 * q + w + 1)]) for w in range(2)]
            for q in range(n)]


def sym_keystream(K, nbytes):
    """SymmetricKey::initialise_encryption (elgamal.rs:175-181): Blake2b-512 of the group element,
    key = h[0..32], nonce = h[32..44], ChaCha20 (IETF, counter 0)."""
    hh = hashlib.blake2b(K, digest_size=64).digest()
    o = buf(nbytes)
    SO.crypto_stream_chacha20_ietf(o, ctypes.c_ulonglong(nbytes), hh[32:44], hh[:32])
    return o.raw


def hybrid_encrypt(pk, r, msg):
    """PublicKey::hybrid_encrypt (elgamal.rs:134-145): e1 = g r, e2 = msg XOR keystream(pk r)."""
    ks = sym_keystream(gmul(pk, r), len(msg))
    return gmul_base(r), bytes(x ^ y for x, y in zip(msg, ks))


def hybrid_decrypt(sk, e1, e2):
    """SecretKey::hybrid_decrypt (elgamal.rs:161-170): keystream(e1 sk) XOR e2."""
    ks = sym_keystream(gmul(e1, sk), len(e2))
    return bytes(x ^ y for x, y in zip(e2, ks))


def from_bits(b32):
    """Scalar::from_bytes = from_bits (groups.rs:29-36): bit 255 cleared; the device reduces mod l."""
    return int.from_bytes(b32, "little") & ((1 << 255) - 1)


def full_ceremony(n, t, master, ceremony_id=0, faults=None):
    """The same ceremony with the shares hybrid-encrypted to the recipients' communication keys
    (committee.rs:164-172) and decrypted by each receiver (committee.rs:282-286,
    procedure_keys.rs:88-105).  Extra faults act on the ciphertexts:
       {"kind": "ct_flip", "dealer": i, "receiver": j, "which": w, "byte": b}  e2 byte b ^= 1,
       {"kind": "e1_generator", "dealer": i, "receiver": j, "which": w}          e1 := g
    with w = 0 (randomness / s' ciphertext) or 1 (share / s ciphertext)."""
    faults = faults or []
    sks, pks = member_keys(master, ceremony_id, n)
    ct_faults = [f for f in faults if f["kind"] in ("ct_flip", "e1_generator")]
    plain_faults = [f for f in faults if f["kind"] in ("share_flip", "rand_flip")]  # before encryption

    def transport(S, SP):
        S = [list(r) for r in S]
        SP = [list(r) for r in SP]
        for f in plain_faults:
            i, j = f["dealer"] - 1, f["receiver"] - 1
            if f["kind"] == "share_flip":
                S[i][j] = (S[i][j] + 1) % L
            else:
                SP[i][j] = (SP[i][j] + 1) % L
        E1 = []
        Sd = [[0] * n for _ in range(n)]
        SPd = [[0] * n for _ in range(n)]
        for i in range(n):
            R = enc_randomness(dealer_seed(master, ceremony_id, i), t, n)
            for q in range(n):
                pair = []
                for w, msg in ((0, SP[i][q]), (1, S[i][q])):   # randomness first (committee.rs:171-172)
                    e1, e2 = hybrid_encrypt(pks[q], R[q][w], scb(msg))
                    for f in ct_faults:
                        if (f["dealer"] - 1, f["receiver"] - 1, f["which"]) == (i, q, w):
                            if f["kind"] == "ct_flip":
                                e2 = e2[:f["byte"]] + bytes([e2[f["byte"]] ^ 1]) + e2[f["byte"] + 1:]
                            else:
                                e1 = gmul_base(1)
                    pair.append((e1, e2))
                    dm = from_bits(hybrid_decrypt(sks[q], e1, e2)) % L
                    if w == 0:
                        SPd[i][q] = dm
                    else:
                        Sd[i][q] = dm
                E1.append(pair)
        extra = {"mode": "full", "member_sk": "".join(hx(scb(x)) for x in sks),
                 "member_pk": "".join(hx(p) for p in pks),
                 "e1": "".join(hx(e1) for pair in E1 for e1, _ in pair),
                 "ct": "".join(hx(e2) for pair in E1 for _, e2 in pair),
                 "enc_r": "".join(hx(scb(x)) for i in range(n)
                                  for rr in enc_randomness(dealer_seed(master, ceremony_id, i), t, n) for x in rr)}
        return Sd, SPd, extra

    other = [f for f in faults if f not in ct_faults and f not in plain_faults]
    out = ceremony(n, t, master, ceremony_id, faults=other, transport=transport)
    out["faults"] = faults
    return out


def kat_hybrid(rng):
    """elgamal.rs hybrid encryption vectors: (pk, r, msg) -> (e1, e2), and back with sk."""
    cases = []
    for k in range(6):
        sk = rng.randrange(1, L)
        pk = gmul_base(sk)
        r = rng.randrange(1, L)
        msg = scb(rng.randrange(L)) if k < 5 else bytes(range(32))
        e1, e2 = hybrid_encrypt(pk, r, msg)
        assert hybrid_decrypt(sk, e1, e2) == msg
        cases.append({"sk": hx(scb(sk)), "pk": hx(pk), "r": hx(scb(r)), "msg": hx(msg), "e1": hx(e1),
                      "e2": hx(e2), "K": hx(gmul(pk, r))})
    seed = member_seed(bytes(32), 0, 0)
    return {"hybrid": cases, "member_seed0": hx(seed),
            "member_sk0": hx(scb(wide_reduce(chacha_stream(seed, 64))))}


# ---------------- complaint proofs: dl_equality/zkp.rs, broadcast.rs ----------------
def hash_to_scalar(data):
    """Scalar::hash_from_bytes::<Blake2b> (groups.rs:50-52): wide reduction of Blake2b-512."""
    return wide_reduce(hashlib.blake2b(data, digest_size=64).digest())


def dleq_prove(b1, b2, p1, p2, dlog, w):
    """DleqZkp::generate (dl_equality/zkp.rs:29-49, challenge_context.rs:14-41)."""
    a1, a2 = gmul(b1, w), gmul(b2, w)
    c = hash_to_scalar(b1 + b2 + p1 + p2 + a1 + a2)
    return c, (c * dlog + w) % L


def dleq_verify(b1, b2, p1, p2, c, r):
    """DleqZkp::verify (dl_equality/zkp.rs:52-74)."""
    a1 = gadd(gmul(b1, r), gneg(gmul(p1, c)))
    a2 = gadd(gmul(b2, r), gneg(gmul(p2, c)))
    return hash_to_scalar(b1 + b2 + p1 + p2 + a1 + a2) == c


def sym_process(K, data):
    ks = sym_keystream(K, len(data))
    return bytes(x ^ y for x, y in zip(data, ks))


def misbehaviour_prove(sk, enc, w):
    """ProofOfMisbehaviour::generate (broadcast.rs:189-226): enc = ((e1_rand, ct_rand), (e1_share,
    ct_share)); the share's decryption proof draws its nonce first (w[0]), the randomness's second."""
    (e1r, _), (e1s, _) = enc
    pk = gmul_base(sk)
    Ks, Kr = gmul(e1s, sk), gmul(e1r, sk)          # recover_symmetric_key (elgamal.rs:154-159)
    g = gmul_base(1)
    c1, r1 = dleq_prove(g, e1s, pk, Ks, sk, w[0])  # CorrectHybridDecrKeyZkp (correct_hybrid.../zkp.rs:27-47)
    c2, r2 = dleq_prove(g, e1r, pk, Kr, sk, w[1])
    return {"share_key": hx(Ks), "randomness_key": hx(Kr), "c1": hx(scb(c1)), "r1": hx(scb(r1)),
            "c2": hx(scb(c2)), "r2": hx(scb(r2))}


def msm_index(j, coeffs, t):
    return msm([pow(j, k, L) for k in range(t + 1)], coeffs)


def complaint1_verify(h, t, j, pk, enc, E, proof):
    """MisbehavingPartiesRound1::verify (broadcast.rs:50-99) incl. ProofOfMisbehaviour::verify
    (:228-283) with its swapped roles (h * share_plaintext + g * randomness_plaintext, :271-274).
    Returns "Ok" or the reference's error name."""
    (e1r, ctr), (e1s, cts) = enc
    g = gmul_base(1)
    Ks, Kr = H(proof["share_key"]), H(proof["randomness_key"])
    ok1 = dleq_verify(g, e1s, pk, Ks, int.from_bytes(H(proof["c1"]), "little"), int.from_bytes(H(proof["r1"]), "little"))
    ok2 = dleq_verify(g, e1r, pk, Kr, int.from_bytes(H(proof["c2"]), "little"), int.from_bytes(H(proof["r2"]), "little"))
    if not (ok1 and ok2):
        return "InvalidProofOfMisbehaviour"
    p1 = from_bits(sym_process(Ks, cts)) % L
    p2 = from_bits(sym_process(Kr, ctr)) % L
    rhs = msm_index(j, E, t)
    if gadd(gmul(h, p1), gmul_base(p2)) == rhs:   # quirk: roles swapped w.r.t. committee.rs:292-294
        return "InvalidProofOfMisbehaviour"
    if gadd(gmul(h, p2), gmul_base(p1)) == rhs:   # the accusation itself (broadcast.rs:76-96)
        return "FalseClaimedInequality"
    return "Ok"


def complaint3_verify(h, t, j, share, rand, E, A):
    """MisbehavingPartiesRound3::verify (broadcast.rs:105-135)."""
    if gadd(gmul_base(share), gmul(h, rand)) != msm_index(j, E, t):
        return "FalseClaimedEquality"
    if gmul_base(share) == msm_index(j, A, t):
        return "FalseClaimedInequality"
    return "Ok"


def H(x):
    return bytes.fromhex(x)


def complaints_golden(full):
    """Proofs and verdicts for every round-2 complaint of a full-mode fault ceremony (and forged
    variants), plus round-3 complaints; nonces from the accuser's member stream (blocks 1 + 2c, 2 + 2c
    for its c-th complaint -- the synthetic convention of this build)."""
    c = full
    n, t = c["n"], c["t"]
    h = H(c["h"])
    sks = [int.from_bytes(H(c["member_sk"])[32 * q:32 * q + 32], "little") for q in range(n)]
    pks = [H(c["member_pk"])[32 * q:32 * q + 32] for q in range(n)]
    master = H(c["master_seed"])
    E = [[H(c["E"])[32 * ((t + 1) * i + k):32 * ((t + 1) * i + k + 1)] for k in range(t + 1)] for i in range(n)]
    e1 = H(c["e1"])
    ct = H(c["ct"])

    def enc(i, q):
        k = 2 * (i * n + q)
        return ((e1[32 * k:32 * k + 32], ct[32 * k:32 * k + 32]), (e1[32 * k + 32:32 * k + 64], ct[32 * k + 32:32 * k + 64]))

    out = []
    for q in range(n):
        accused = [i for i in range(n) if i != q and c["dec2"][i * n + q] == "0"]
        # accuser q's member seed order: the member index before sorting is not needed: the nonce
        # stream is keyed by the SORTED index q (this build's convention)
        st = chacha_stream(member_seed(master, c["ceremony"], 1000 + q), 64 * (1 + 2 * max(1, len(accused)) + 2))
        for ci, i in enumerate(accused):
            w = [wide_reduce(st[64 * (1 + 2 * ci + k):64 * (2 + 2 * ci + k)]) for k in range(2)]
            proof = misbehaviour_prove(sks[q], enc(i, q), w)
            verdict = complaint1_verify(h, t, q + 1, pks[q], enc(i, q), E[i], proof)
            assert verdict == "Ok", (q, i, verdict)
            out.append({"accuser": q + 1, "accused": i + 1, "w": [hx(scb(x)) for x in w], "proof": proof,
                        "verdict": verdict})
    # forged complaints: an honest pair (proof valid, inequality false) and a tampered proof
    qs, ivs = 0, 1
    st = chacha_stream(member_seed(master, c["ceremony"], 2000), 128)
    w = [wide_reduce(st[:64]), wide_reduce(st[64:])]
    proof = misbehaviour_prove(sks[qs], enc(ivs, qs), w)
    out.append({"accuser": qs + 1, "accused": ivs + 1, "w": [hx(scb(x)) for x in w], "proof": proof,
                "verdict": complaint1_verify(h, t, qs + 1, pks[qs], enc(ivs, qs), E[ivs], proof)})
    bad = dict(proof)
    bad["r1"] = hx(scb(int.from_bytes(H(proof["r1"]), "little") + 1))
    out.append({"accuser": qs + 1, "accused": ivs + 1, "w": [hx(scb(x)) for x in w], "proof": bad,
                "verdict": complaint1_verify(h, t, qs + 1, pks[qs], enc(ivs, qs), E[ivs], bad)})
    return out


def complaints3_golden(c):
    """Round-3 complaints of a plaintext ceremony (MisbehavingPartiesRound3, broadcast.rs:105-135):
    every receiver's complaint against each accused dealer, plus a forged one."""
    n, t = c["n"], c["t"]
    h = H(c["h"])
    E = [[H(c["E"])[32 * ((t + 1) * i + k):32 * ((t + 1) * i + k + 1)] for k in range(t + 1)] for i in range(n)]
    A = [[H(c["A"])[32 * ((t + 1) * i + k):32 * ((t + 1) * i + k + 1)] for k in range(t + 1)] for i in range(n)]
    s, sp = H(c["s"]), H(c["s_prime"])
    out = []
    for i in range(n):
        for j in range(n):
            if i == j or c["dec4"][i * n + j] != "0":
                continue
            sh, ra = int.from_bytes(s[32 * (i * n + j):32 * (i * n + j) + 32], "little"), \
                int.from_bytes(sp[32 * (i * n + j):32 * (i * n + j) + 32], "little")
            out.append({"accuser": j + 1, "accused": i + 1, "share": hx(scb(sh)), "randomness": hx(scb(ra)),
                        "verdict": complaint3_verify(h, t, j + 1, sh, ra, E[i], A[i])})
    # forged: an honest dealer's pair (FalseClaimedInequality) and a wrong share (FalseClaimedEquality)
    i, j = 1, 2
    sh = int.from_bytes(s[32 * (i * n + j):32 * (i * n + j) + 32], "little")
    ra = int.from_bytes(sp[32 * (i * n + j):32 * (i * n + j) + 32], "little")
    out.append({"accuser": j + 1, "accused": i + 1, "share": hx(scb(sh)), "randomness": hx(scb(ra)),
                "verdict": complaint3_verify(h, t, j + 1, sh, ra, E[i], A[i])})
    out.append({"accuser": j + 1, "accused": i + 1, "share": hx(scb(sh + 1)), "randomness": hx(scb(ra)),
                "verdict": complaint3_verify(h, t, j + 1, sh + 1, ra, E[i], A[i])})
    return out


def kat_group(rng):
    out = {}
    out["base_multiples"] = [{"k": k, "P": hx(gmul_base(k))} for k in range(0, 17)]
    ks = [rng.randrange(L) for _ in range(8)] + [L - 1, L - 2, 2**252, 2**128 + 7]
    out["base_mul"] = [{"k": hx(scb(k)), "P": hx(gmul_base(k))} for k in ks]
    for k in ks[:4]:
        assert r255.encode(r255.mul(r255.BASE, k)) == gmul_base(k)
    out["hash_to_group"] = [{"msg": hx(m), "P": hx(hash_to_group(m))}
                            for m in [CK_BYTES, b"\x00", b"", bytes(range(200))]]
    uni = []
    for _ in range(8):
        u = bytes(rng.getrandbits(8) for _ in range(64))
        o = buf(32)
        SO.crypto_core_ristretto255_from_hash(o, u)
        assert r255.encode(r255.from_uniform_bytes(u)) == o.raw
        uni.append({"in": hx(u), "P": hx(o.raw)})
    out["from_uniform_bytes"] = uni
    adds = []
    for _ in range(8):
        p, q = gmul_base(rng.randrange(L)), gmul_base(rng.randrange(L))
        adds.append({"P": hx(p), "Q": hx(q), "sum": hx(gadd(p, q)), "diff": hx(gadd(p, gneg(q))),
                     "neg_P": hx(gneg(p))})
    out["add"] = adds
    muls = []
    for _ in range(8):
        p, k = gmul_base(rng.randrange(L)), rng.randrange(L)
        muls.append({"P": hx(p), "k": hx(scb(k)), "kP": hx(gmul(p, k))})
    out["mul"] = muls
    # encodings that must fail to decode (CompressedRistretto::decompress -> None)
    P = r255.P
    bad = [(P).to_bytes(32, "little"), (P + 2).to_bytes(32, "little"), (2**255 - 2).to_bytes(32, "little"),
           (1).to_bytes(32, "little"), bytes([0xff] * 32), bytes(31) + b"\x80"]
    for _ in range(40):
        cand = bytes(rng.getrandbits(8) for _ in range(32))
        if not valid(cand) and cand not in bad:
            bad.append(cand)
        if len(bad) >= 16:
            break
    for b in bad:
        # dalek (and RFC 9496) reject a set bit 255 via the canonical re-encoding check;
        # libsodium 1.0.18 masks that bit in its canonicity test, so it only arbitrates the rest.
        assert r255.decode(b) is None, b.hex()
        assert b[31] & 0x80 or not valid(b), b.hex()
    out["invalid_encodings"] = [hx(b) for b in bad]
    # MSM (vartime_multiscalar_multiplication) at sizes on both sides of dalek's Straus/Pippenger
    # switch (190) and window thresholds (500, 800)
    cases = []
    for N in [0, 1, 2, 5, 32, 189, 190, 256, 512]:
        sc = [rng.randrange(L) for _ in range(N)]
        pts = [gmul_base(rng.randrange(L)) for _ in range(N)]
        cases.append({"N": N, "scalars": "".join(hx(scb(x)) for x in sc),
                      "points": "".join(hx(p) for p in pts), "out": hx(msm(sc, pts))})
    # a vector with identity points and zero / l-1 scalars (fault-injection shapes)
    sc = [0, 1, L - 1, 5]
    pts = [ID, gmul_base(3), gmul_base(9), ID]
    cases.append({"N": 4, "scalars": "".join(hx(scb(x)) for x in sc), "points": "".join(hx(p) for p in pts),
                  "out": hx(msm(sc, pts))})
    out["msm"] = cases
    return out


def kat_scalar(rng):
    out = {}
    wides = [bytes([0xff] * 64), bytes(64), (L).to_bytes(64, "little"), (2 * L + 5).to_bytes(64, "little")]
    wides += [bytes(rng.getrandbits(8) for _ in range(64)) for _ in range(8)]
    out["reduce_wide"] = [{"in": hx(w), "out": hx(scb(int.from_bytes(w, "little")))} for w in wides]
    ops = []
    for _ in range(12):
        a, b = rng.randrange(L), rng.randrange(L)
        ops.append({"a": hx(scb(a)), "b": hx(scb(b)), "add": hx(scb(a + b)), "sub": hx(scb(a - b)),
                    "mul": hx(scb(a * b)), "neg_a": hx(scb(-a)), "inv_a": hx(scb(pow(a, -1, L)))})
    out["ops"] = ops
    # polynomial.rs:240-279 KATs
    out["poly_tests"] = {"coeffs": [1, 3, 0, 0, 0], "x": 3, "value": 10}
    # polynomial.rs:190-211: 13 + 2x through x in {5, 7, 2}
    xs = [5, 7, 2]
    ys = [evaluate([13, 2], x) for x in xs]
    out["lagrange"] = {"xs": xs, "ys": ys, "at_zero": lagrange_at_zero(ys, xs)}
    evals = []
    for deg in [0, 1, 4, 31, 127]:
        c = [rng.randrange(L) for _ in range(deg + 1)]
        xs = [1, 2, 3, 1023, 4096, rng.randrange(1, 2**32)]
        evals.append({"coeffs": "".join(hx(scb(x)) for x in c),
                      "points": xs, "values": [hx(scb(evaluate(c, x))) for x in xs]})
    out["poly_eval"] = evals
    # the RNG convention (committee.rs:143-146 draw order) on one seed
    seed = dealer_seed(bytes(32), 0, 0)
    a, b = dealer_coeffs(seed, 3)
    out["dealer_rng"] = {"master": hx(bytes(32)), "ceremony": 0, "dealer": 0, "seed": hx(seed), "t": 3,
                         "a": [hx(scb(x)) for x in a], "b": [hx(scb(x)) for x in b],
                         "stream_head": hx(chacha_stream(seed, 128))}
    return out


def spot(n, t, master, dealers, receivers):
    """Per-pair spot vectors for a large config: full E/A of a few dealers plus chosen shares."""
    h = hash_to_group(CK_BYTES)
    res = {"n": n, "t": t, "master_seed": hx(master), "h": hx(h), "dealers": []}
    for i in dealers:
        a, b = dealer_coeffs(dealer_seed(master, 0, i), t)
        ap = [gmul_base(x) for x in a]
        E = [gadd(gmul(h, y), x) for x, y in zip(ap, b)]
        d = {"dealer": i, "E": "".join(hx(p) for p in E), "A": "".join(hx(p) for p in ap), "pairs": []}
        for j in receivers:
            s, sp = evaluate(a, j + 1), evaluate(b, j + 1)
            pw = [pow(j + 1, k, L) for k in range(t + 1)]
            rhs2, rhs4 = msm(pw, E), msm(pw, ap)
            assert rhs2 == gadd(gmul(h, sp), gmul_base(s)) and rhs4 == gmul_base(s)
            d["pairs"].append({"receiver": j, "s": hx(scb(s)), "s_prime": hx(scb(sp)), "rhs2": hx(rhs2)})
        res["dealers"].append(d)
    return res


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = random.Random(20250117)
    files = {}
    files["kat_group.json"] = kat_group(rng)
    files["kat_scalar.json"] = kat_scalar(rng)
    m = hashlib.blake2b(b"golden/master", digest_size=32).digest()
    for n, t in [(2, 0), (3, 1), (10, 4), (11, 5), (16, 7)]:
        files[f"ceremony_n{n}_t{t}.json"] = ceremony(n, t, m)
    files["ceremony_n64_t31.json"] = ceremony(64, 31, m, ceremony_id=7, with_coeffs=False)
    faults = {
        "e_identity": [{"kind": "E_identity", "dealer": 3}],
        "share_flip": [{"kind": "share_flip", "dealer": 5, "receiver": 2},
                       {"kind": "rand_flip", "dealer": 7, "receiver": 9}],
        "a_generator": [{"kind": "A_generator", "dealer": 6}],
        "over_threshold": [{"kind": "E_identity", "dealer": d} for d in (1, 2, 4, 8, 9)],
        "a_many": [{"kind": "A_generator", "dealer": d} for d in (1, 3, 5, 6, 8, 10)],
    }
    for name, fs in faults.items():
        files[f"fault_{name}_n10_t4.json"] = ceremony(10, 4, m, ceremony_id=1, faults=fs)
    files["kat_hybrid.json"] = kat_hybrid(random.Random(7))
    files["full_n4_t1.json"] = full_ceremony(4, 1, m, ceremony_id=3)
    files["full_n10_t4.json"] = full_ceremony(10, 4, m, ceremony_id=4)
    files["full_faults_n10_t4.json"] = full_ceremony(10, 4, m, ceremony_id=4, faults=[
        {"kind": "ct_flip", "dealer": 3, "receiver": 5, "which": 1, "byte": 7},
        {"kind": "e1_generator", "dealer": 6, "receiver": 2, "which": 0},
        {"kind": "share_flip", "dealer": 9, "receiver": 1}])
    ff = files["full_faults_n10_t4.json"]
    files["complaints_n10_t4.json"] = {
        "source": "full_faults_n10_t4.json", "round1": complaints_golden(ff),
        "round3_source": "fault_a_generator_n10_t4.json",
        "round3": complaints3_golden(files["fault_a_generator_n10_t4.json"])}
    files["spot_n256_t127.json"] = spot(256, 127, m, [0, 200], [1, 17, 255])
    files["spot_n1024_t511.json"] = spot(1024, 511, m, [513], [0, 1023])
    # the dealer's unchecked share to itself (s_ii) tampered, plus an A fault on the same dealer (i <= t):
    # reconstructed in finalise, where s_ii must not be used; and a second reconstructed dealer
    files["fault_self_share_n10_t4.json"] = ceremony(10, 4, m, ceremony_id=2, faults=[
        {"kind": "self_share_flip", "dealer": 2}, {"kind": "A_generator", "dealer": 2},
        {"kind": "A_generator", "dealer": 7}, {"kind": "E_identity", "dealer": 9}])
    fs = files["fault_self_share_n10_t4.json"]
    n10 = 10
    cases = [
        {"name": "all disclose"},
        {"name": "t points (4 final parties disclose)", "disclosed": [1 if j in (0, 2, 3, 4) else 0 for j in range(n10)]},
        {"name": "t-1 points", "disclosed": [1 if j in (0, 3, 4) else 0 for j in range(n10)]},
        {"name": "none disclose", "disclosed": [0] * n10},
        {"name": "earlier failures", "r2_error": [1 if j == 5 else 0 for j in range(n10)],
         "r4_error": [1 if j == 0 else 0 for j in range(n10)]},
    ]
    files["finalise_parties_n10_t4.json"] = {"source": "fault_self_share_n10_t4.json",
                                             "cases": finalise_golden(fs, cases)}
    # no disqualified dealer: the per-party view without the reference's finalise panic
    files["fault_recon_only_n10_t4.json"] = ceremony(10, 4, m, ceremony_id=5, faults=[
        {"kind": "self_share_flip", "dealer": 3}, {"kind": "A_generator", "dealer": 3},
        {"kind": "A_generator", "dealer": 8}])
    fr = files["fault_recon_only_n10_t4.json"]
    files["finalise_parties_recon_n10_t4.json"] = {"source": "fault_recon_only_n10_t4.json", "cases": finalise_golden(fr, [
        {"name": "all disclose"},
        {"name": "t points", "disclosed": [1 if j in (0, 1, 3, 4) else 0 for j in range(n10)]},
        {"name": "t-1 points", "disclosed": [1 if j in (0, 1, 4) else 0 for j in range(n10)]},
        {"name": "one missing", "disclosed": [0 if j == 5 else 1 for j in range(n10)]},
        # four final parties stop at Phase3 (r4_error) and never disclose: the others are left with
        # exactly t points although every disclosure flag is set (a wrong secret, as the reference)
        {"name": "r4 errors leave t points", "r4_error": [1 if j in (0, 1, 3, 4) else 0 for j in range(n10)]},
        {"name": "r2 and r4 errors leave t-1 points",
         "r2_error": [1 if j in (0, 1) else 0 for j in range(n10)],
         "r4_error": [1 if j in (3, 4, 5) else 0 for j in range(n10)]}])}
    # final parties with round-2 errors never disclose in phase 5 (committee.rs:340-347, 684): dealers
    # 1-4 send bad shares to 8 (then 9) receivers, who raise more than t complaints; dealer 16's
    # round-3 commitments are wrong, so it is reconstructed from the remaining final parties'
    # disclosures -- exactly t of them (a wrong secret, as the reference computes it), then t-1
    # (InsufficientSharesForRecovery for every finalising party: no mpk)
    for name, last in (("fault_recon_r2err_n16_t3.json", 12), ("fault_recon_insufficient_n16_t3.json", 13)):
        files[name] = ceremony(16, 3, m, ceremony_id=8, faults=[
            {"kind": "share_flip", "dealer": d, "receiver": j} for d in range(1, 5) for j in range(5, last + 1)] + [
            {"kind": "A_generator", "dealer": 16}])
    files["spot_n4096_t2047.json"] = spot(4096, 2047, m, [5, 3000], [0, 1500, 4095])
    # n = 8: a ceremony under a commitment key of its own (h and its comb differ from every other
    # fixture's) and a full-mode ceremony with its own member keys (tests/test_gpu_comb_build.py)
    files["ceremony_n8_t3_ck.json"] = ceremony(8, 3, m, ceremony_id=9, ck=b"A commitment key of this ceremony's own.")
    files["full_n8_t3.json"] = full_ceremony(8, 3, m, ceremony_id=10)
    only = set(sys.argv[1].split(",")) if len(sys.argv) > 1 else None
    files = {k: v for k, v in files.items() if only is None or k in only}
    for obj in files.values():
        obj.pop("_state", None)
    for name, obj in files.items():
        with open(os.path.join(OUT, name), "w") as f:
            json.dump(obj, f, separators=(",", ":"))
        print(name, os.path.getsize(os.path.join(OUT, name)))


if __name__ == "__main__":
    main()
