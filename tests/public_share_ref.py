"""Checker (test infrastructure only): the public shares g s_j of a ceremony from its public data, on
Python integers over tests/ristretto_ref.py -- a model of dkg_commitment_sum, dkg_public_share_status and
dkg_public_shares.

    public_share[j] = sum_{i qualified, not reconstructed} sum_k (j+1)^k A_i[k]  +  g sum_{i reconstructed} s_ij

The dealers that stay passed round 4, g s_ij = sum_k (j+1)^k A_i[k] (committee.rs:532-539), and s_j is the sum
of their s_ij and of the reconstructed dealers' (committee.rs:453-461: every qualified dealer); a
reconstructed dealer's share is the one party j disclosed in phase 5 (BroadcastPhase5, :660-669).  Pinned
against the libsodium fixtures by tests/test_public_share_ref.py.
"""
from tests import ristretto_ref as R

OK, NO_COMMITMENT, NO_DISCLOSURE = 0, 1, 2
ZERO = bytes(32)

_decoded = {}


def decode(b):
    b = bytes(b)
    if b not in _decoded:
        _decoded[b] = R.decode(b)
    return _decoded[b]


def row(A, t, r):
    """The t + 1 encodings of row r of A [rows][t+1][32]."""
    N = t + 1
    return [A[32 * (r * N + k):32 * (r * N + k) + 32] for k in range(N)]


def commitment_sum(B, n, t, A, mask=None):
    """(S [B][t+1][32], ok [B]): the masked column sums; a masked row that does not decode zeroes the ceremony."""
    N = t + 1
    S, ok = [], []
    for c in range(B):
        acc, good = [R.IDENTITY] * N, 1
        for i in range(n):
            if mask is not None and not mask[c * n + i]:
                continue
            pts = [decode(x) for x in row(A, t, c * n + i)]
            if any(p is None for p in pts):
                good = 0
                continue
            acc = [R.add(a, p) for a, p in zip(acc, pts)]
        ok.append(good)
        S.append(b"".join(R.encode(a) for a in acc) if good else ZERO * N)
    return b"".join(S), ok


def status(n, qualified, reconstruct, j, pairs, a_present=None):
    """(status, which) of index j (0-based) of one ceremony; pairs: the (sender, dealer) disclosures, 1-based."""
    reconstruct = reconstruct or [0] * n
    for i in range(n):
        if qualified[i] and not reconstruct[i] and a_present is not None and not a_present[i]:
            return NO_COMMITMENT, i
    have = set(pairs)
    for i in range(n):
        if reconstruct[i] and (j + 1, i + 1) not in have:
            return NO_DISCLOSURE, i
    return OK, -1


def public_shares(B, n, t, A, qualified, js, reconstruct=None, disclosures=(), fetched3=None):
    """(V [B][M][32], status [B*M], which [B*M], S [B][t+1][32]); disclosures: (ceremony, sender, dealer,
    share bytes) with sender / dealer 1-based."""
    N, M = t + 1, len(js)
    reconstruct = reconstruct or [0] * (B * n)
    mask = [int(bool(qualified[e]) and not reconstruct[e]) for e in range(B * n)]
    present = []
    for e in range(B * n):
        p = fetched3 is None or bool(fetched3[e])
        if p and mask[e]:
            p = all(decode(x) is not None for x in row(A, t, e))
        present.append(int(p))
    S, _ = commitment_sum(B, n, t, A, [m and p for m, p in zip(mask, present)])
    shares = {(c, q, i): R.from_bits(s) for c, q, i, s in disclosures}
    V, st, wh = [], [], []
    for c in range(B):
        sl = slice(c * n, (c + 1) * n)
        pairs = [(q, i) for (g, q, i) in shares if g == c]
        coeffs = [decode(x) for x in row(S, t, c)]
        for j in js:
            s, w = status(n, qualified[sl], reconstruct[sl], j, pairs, present[sl])
            st.append(s)
            wh.append(w)
            if s != OK:
                V.append(ZERO)
                continue
            acc = R.IDENTITY
            for k in reversed(range(N)):
                acc = R.add(R.mul(j + 1, acc), coeffs[k])
            disclosed = sum(shares[(c, j + 1, i + 1)] for i in range(n) if reconstruct[c * n + i]) % R.L
            V.append(R.encode(R.add(acc, R.mul(disclosed, R.BASE))))
    # S as dkg_public_shares reports it: the call's mask, a ceremony with an unusable used row zeroed
    Sout = b"".join(ZERO * N if any(mask[e] and not present[e] for e in range(c * n, (c + 1) * n))
                    else S[32 * N * c:32 * N * (c + 1)] for c in range(B))
    return b"".join(V), st, wh, Sout


def fixture_disclosures(c, ceremony=0):
    """Every party's phase-5 disclosure of a fixture: s[i][j] for every reconstructed dealer i and every j."""
    n, s = c["n"], bytes.fromhex(c["s"])
    return [(ceremony, j + 1, i + 1, s[32 * (i * n + j):32 * (i * n + j) + 32])
            for i in range(n) if c["reconstruct"][i] for j in range(n)]
