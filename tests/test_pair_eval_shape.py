"""dkg_pair_eval_shape (host only) and a scalar model of k_pair_eval's lane schedule over Z_l: the chunks
with their identity-padded steps, the migrating fold with the partner at u - 2^s, the result in lane
2^S - 1, the multipliers of dkg_receiver_plan_for(.., chunk = L).  Pins the exponent bookkeeping of the
wave evaluator without a GPU."""
import random

import pytest

import dkg_amd
from dkg_amd import DkgError

ELL = 2**252 + 27742317777372353535851937790883648493


def ceil_log2(g):
    s = 0
    while (1 << s) < g:
        s += 1
    return s


@pytest.mark.parametrize("N", list(range(1, 301)) + [512, 2048])
def test_automatic_shape(N):
    sh = dkg_amd.pair_eval_shape(N - 1)
    L, lanes, stages = sh["chunk"], sh["lanes"], sh["stages"]
    assert L == -(-N // 64)
    assert 1 <= lanes <= 64
    assert L * lanes >= N
    assert (lanes - 1) * L < N
    assert stages == ceil_log2(lanes)


@pytest.mark.parametrize("N, chunk, lanes", [(1, 1, 1), (1, 7, 1), (8, 1, 8), (8, 2, 4), (8, 3, 3), (8, 8, 1),
                                              (8, 64, 1), (128, 2, 64), (128, 3, 43), (128, 5, 26), (128, 128, 1),
                                              (129, 3, 43), (512, 8, 64), (512, 9, 57), (4096, 64, 64)])
def test_forced_shape(N, chunk, lanes):
    sh = dkg_amd.pair_eval_shape(N - 1, chunk)
    assert sh == {"chunk": min(chunk, N), "lanes": lanes, "stages": ceil_log2(lanes)}


@pytest.mark.parametrize("N, chunk", [(65, 1), (129, 2), (512, 7), (2048, 31), (8, -1)])
def test_rejected_shape(N, chunk):
    with pytest.raises(DkgError):
        dkg_amd.pair_eval_shape(N - 1, chunk)


def test_null_outputs():
    import ctypes

    L = dkg_amd.lib()
    v = ctypes.c_uint32()
    for k in range(3):
        args = [ctypes.byref(v)] * 3
        args[k] = None
        assert L.dkg_pair_eval_shape(7, 0, *args) != 0


def wave_model(coeffs, x, chunk):
    """What lane 2^S - 1 of k_pair_eval holds, with integers mod l in the points' place (identity = 0)."""
    N = len(coeffs)
    sh = dkg_amd.pair_eval_shape(N - 1, chunk)
    L, G, S = sh["chunk"], sh["lanes"], sh["stages"]
    mult = []
    if S:
        plan = dkg_amd.receiver_plan(x, N - 1, x, L)
        assert plan["chunk"] == L and plan["stages"] == S and plan["arity"] == [2] * S
        mult = plan["mult"]
    V = []
    for u in range(64):
        k = u * L + L - 1
        acc = coeffs[k] if u < G and k < N else 0
        for i in reversed(range(L - 1)):  # the same L - 1 steps in every lane
            k = u * L + i
            acc = (acc * x + (coeffs[k] if u < G and k < N else 0)) % ELL
        V.append(acc)
    for s in range(S):
        col = list(V)  # the LDS columns: every lane's value before the stage's multiplication
        w = 1 << s
        V = [(mult[s] * V[u] + (col[u - w] if u & w else col[u])) % ELL for u in range(64)]
    return V[(1 << S) - 1]


CHUNKS = {1: [0, 1, 4], 2: [0, 1, 2, 5], 3: [0, 1, 2, 3], 64: [0, 1, 3, 5, 64], 65: [0, 2, 3, 7, 65],
          129: [0, 3, 4, 11, 128, 200], 512: [0, 8, 9, 11, 100, 511]}


@pytest.mark.parametrize("N", sorted(CHUNKS))
def test_wave_model(N):
    rng = random.Random(1000 + N)
    coeffs = [rng.randrange(ELL) for _ in range(N)]
    for x in (1, 2, 3, 683, 1024):
        exp = sum(pow(x, k, ELL) * c for k, c in enumerate(coeffs)) % ELL
        for chunk in CHUNKS[N]:
            assert wave_model(coeffs, x, chunk) == exp, (x, chunk)
