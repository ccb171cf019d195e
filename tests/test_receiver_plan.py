"""dkg_receiver_plan_for: the host-only plan of one party's chunked evaluation (no GPU).  The replay of
a plan over Z_l lives here, not in the library."""
import random

import pytest

import dkg_amd
from dkg_amd import DkgError

L = 2**252 + 27742317777372353535851937790883648493


def naf_cost(m):
    """c(m) = NAF length - 1 + NAF weight - 1 (doublings + additions of the chain; 0 for m = 1)."""
    if m <= 1:
        return 0
    return ((3 * m).bit_length() - 1) - 1 + bin((3 * m ^ m) >> 1).count("1") - 1


def chain(p, x):
    return (p["chunk"] - 1) * (naf_cost(x) + 1) + sum((r - 1) * (naf_cost(y) + 1) for r, y in zip(p["arity"], p["mult"]))


def check_plan(n, t, x, chunk):
    N = t + 1
    p = dkg_amd.receiver_plan(n, t, x, chunk)
    if chunk:
        assert p["chunk"] == chunk
    assert p["chunk"] >= 1 and p["stages"] <= 16
    if p["chunk"] >= N:
        assert p["stages"] == 0
        return p
    Lc = p["chunk"]
    G = -(-N // Lc)
    assert all(r >= 2 for r in p["arity"]) and all(y < 2**255 for y in p["mult"])
    if G > 1:
        assert p["mult"][0] % L == pow(x, Lc, L)
    for s in range(p["stages"] - 1):
        assert p["mult"][s + 1] % L == pow(p["mult"][s], p["arity"][s], L)
    prod = 1
    for r in p["arity"]:
        prod *= r
    assert prod >= G
    # replay over Z_l on random "coefficients"
    rnd = random.Random(n * 1000003 + t * 101 + x + chunk)
    for _ in range(2):
        c = [rnd.randrange(L) for _ in range(N)]
        q = [sum(c[u * Lc + k] * pow(x, k, L) for k in range(min(Lc, N - u * Lc))) % L for u in range(G)]
        for r, y in zip(p["arity"], p["mult"]):
            q = [sum(q[v + i] * pow(y, i, L) for i in range(min(r, len(q) - v))) % L for v in range(0, len(q), r)]
        assert len(q) == 1, "the last stage must leave one value"
        assert q[0] == sum(ck * pow(x, k, L) for k, ck in enumerate(c)) % L
    return p


EDGE = [
    (2, 0, 1, 0), (2, 0, 2, 3),                      # N = 1
    (10, 4, 7, 1), (1024, 511, 683, 1),              # chunk 1: fold only
    (130, 64, 129, 65), (130, 64, 129, 70),          # chunk = N, chunk > N: serial
    (130, 64, 130, 8), (130, 64, 3, 64),             # ragged last chunk
    (48, 23, 48, 8), (80, 39, 2, 8), (144, 71, 143, 8),  # G = 3, 5, 9
    (4096, 3, 4096, 2), (4096, 3, 4095, 0), (8192, 2047, 4096, 16),
]


@pytest.mark.parametrize("n,t,x,chunk", EDGE)
def test_plan_edges(n, t, x, chunk):
    check_plan(n, t, x, chunk)


def test_plan_random():
    rnd = random.Random(7)
    for _ in range(150):
        n = rnd.choice([2, 3, 10, 64, 65, 130, 256, 1024, 4096, 5000])
        t = rnd.randrange(0, (n + 1) // 2)
        x = rnd.choice([1, 2, n, max(1, n - 1), min(n, 4096), rnd.randrange(1, n + 1)])
        chunk = rnd.choice([0, 0, 1, 2, 3, 5, 8, 16, 64, t + 1, t + 6])
        check_plan(n, t, x, chunk)


@pytest.mark.parametrize("n,t,dense,bound", [(1024, 511, 683, 0.35), (4096, 2047, 2731, 0.10),
                                             (1024, 3, 683, 1.0), (64, 31, 43, 1.0)])
def test_automatic_chain_bound(n, t, dense, bound):
    """The automatic plan's dependent chain against the serial walk's (N - 1)(c(x) + 1): the binary tree
    at chunk 8 gives 1,665-1,752 of 5,621-8,176 at (1024, 511) and 2,393-2,519 of 26,611-38,893 at
    (4096, 2047); the bounds are those ratios with a small allowance."""
    for x in (n, n - 1, dense):
        p = check_plan(n, t, x, 0)
        serial = t * (naf_cost(x) + 1)
        got = chain(p, x) if p["stages"] else (t * (naf_cost(x) + 1))
        assert got <= bound * serial, (n, t, x, p["chunk"], got, serial)


def test_plan_argument_errors():
    for args in [(10, 4, 0, 0), (10, 4, 11, 0), (10, 4, 3, -1), (0, 0, 1, 0)]:
        with pytest.raises(DkgError) as e:
            dkg_amd.receiver_plan(*args)
        assert e.value.code == -1
    assert dkg_amd.lib().dkg_receiver_plan_for(10, 4, 3, 0, None) == -1
    # more than 16 binary stages
    with pytest.raises(DkgError):
        dkg_amd.receiver_plan(2**20, 2**18, 5, 1)
    # the plan does not apply the environment's t < (n + 1) / 2 guard (stated in dkg_amd.h)
    assert dkg_amd.receiver_plan(10, 9, 3, 4)["chunk"] == 4
    c = dkg_amd.receiver_plan_constants()
    assert all(v > 0 for v in c.values())
