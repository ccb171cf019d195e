"""dkg_seat_eval_shape (host only): the shape the seats calls evaluate in -- forced chunks against the
formulas and dkg_receiver_plan_for, the automatic rule's guarantees, and what it returns for the shapes
of profiles/seats_time.json and profiles/seat_chunks_time.json."""
import json
import os

import pytest

import dkg_amd
from dkg_amd import DkgError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GIB = 1 << 30


def ceil_log2(g):
    return (g - 1).bit_length()


@pytest.mark.parametrize("N", [1, 2, 5, 32, 65, 512])
def test_forced_chunks(N):
    t, n = N - 1, 2 * N + 1
    for chunk in (1, 2, 3, N - 1, N, N + 5):
        if chunk < 1:
            continue
        for waves, x in ((1, 1), (3, n), (16, 2)):
            r = dkg_amd.seat_eval_shape(n, t, waves, x, chunk)
            L = min(chunk, N)
            G = -(-N // L)
            assert (r["chunk"], r["chunks"], r["stages"]) == (L, G, ceil_log2(G)), (N, chunk)
            assert r["stages"] == dkg_amd.receiver_plan(n, t, x, chunk)["stages"]
            assert r["scratch_bytes"] == (2 * 160 * G * 64 * waves if G > 1 else 0)


def test_forced_scratch_is_reported_not_refused():
    """A forced shape above 1 GiB is still a shape: the call refuses it, the pure function reports the size."""
    r = dkg_amd.seat_eval_shape(4096, 2047, 4096, 7, 1)
    assert r["chunks"] == 2048 and r["scratch_bytes"] == 2 * 160 * 2048 * 64 * 4096 > GIB


def serial_chain(N, x):
    return (N - 1) * (chain_ops(x) + 1)


def chain_ops(m):
    """doublings + additions of the NAF chain of m (1: none), as the rule counts them"""
    if m <= 1:
        return 0
    length = weight = 0
    i = 0
    while m:
        if m & 1:
            d = 2 - (m & 3)
            m -= d
            weight += 1
            length = i + 1
        m >>= 1
        i += 1
    return (length - 1) + (weight - 1)


SHAPES = [(n, t, w, x) for (n, t) in ((2, 0), (3, 1), (10, 4), (16, 7), (64, 31), (130, 64), (256, 127), (1024, 511),
                                      (4096, 2047))
          for w in (1, 2, 16, 64, 1000, 40000) for x in sorted({1, 2, 3, n // 2 + 1, n - 1, n}) if 1 <= x <= n]


def test_automatic_guarantees():
    ell = 2**252 + 27742317777372353535851937790883648493
    for n, t, w, x in SHAPES:
        N = t + 1
        r = dkg_amd.seat_eval_shape(n, t, w, x)
        L, G = r["chunk"], r["chunks"]
        assert r["scratch_bytes"] <= GIB
        if G == 1:
            assert (L, r["stages"], r["scratch_bytes"]) == (N, 0, 0)
            continue
        assert L in (2, 4, 8, 16, 32, 64) and L < N and G == -(-N // L) and r["stages"] == ceil_log2(G)
        assert r == dkg_amd.seat_eval_shape(n, t, w, x, L)  # the forced shape of the same function
        chain = (L - 1) * (chain_ops(x) + 1)
        y = pow(x, L, ell)
        for _ in range(r["stages"]):
            chain += chain_ops(y) + 1
            y = y * y % ell
        assert chain <= serial_chain(N, x), (n, t, w, x)


def test_measured_shapes_stay_serial():
    """Every (n, t, waves) row of profiles/seats_time.json -- (64, 31) and (16, 7) at every S -- stays on
    k_seat_horner, whatever the largest index, with the one exception profiles/seat_chunks_time.json shows
    beyond the repetitions' spread: (64, 31) at S = 1 and 16 (1 and 16 waves), where a chunked shape is
    0.12-0.13 ms below the serial walk's 0.92 / 1.05 ms and the rule may take it."""
    with open(os.path.join(ROOT, "profiles", "seats_time.json")) as f:
        rec = json.load(f)
    rows = 0
    for key in ("n64", "n16"):
        n, t = rec[key]["n"], rec[key]["t"]
        for row in rec[key]["rows"]:
            rows += 1
            if n == 64 and row["waves"] <= 16:
                continue
            for x in range(1, n + 1):
                r = dkg_amd.seat_eval_shape(n, t, row["waves"], x)
                assert (r["chunk"], r["chunks"], r["stages"]) == (t + 1, 1, 0), (n, row["seats"], x)
    assert rows == 10
    with open(os.path.join(ROOT, "profiles", "seat_chunks_time.json")) as f:
        new = {(p["n"], p["seats"]): p for p in json.load(f)["points"]}
    for S in (1, 16):  # the exception is the record's, not the rule's
        w = new[(64, S)]["wall_ms"]
        assert min(w[k]["max"] for k in w if k.startswith("mode2_L")) < w["mode1"]["min"]


def test_record_supports_the_rule():
    """The automatic choice against profiles/seat_chunks_time.json: wherever the record shows the best forced
    chunk below the serial walk with disjoint min-max ranges, the rule leaves the serial walk, and it never
    does where the serial walk is the faster by that measure."""
    with open(os.path.join(ROOT, "profiles", "seat_chunks_time.json")) as f:
        rec = json.load(f)
    seen = 0
    for point in rec["points"]:
        n, t, waves, x_max = point["n"], point["t"], point["waves"], point["x_max"]
        w = point["wall_ms"]
        forced = {k: v for k, v in w.items() if k.startswith("mode2_L")}
        best = min(forced.values(), key=lambda v: v["median"])
        r = dkg_amd.seat_eval_shape(n, t, waves, x_max)
        if best["max"] < w["mode1"]["min"]:
            assert r["chunks"] > 1, (n, point["seats"])
            seen += 1
        elif w["mode1"]["max"] < best["min"]:
            assert r["chunks"] == 1, (n, point["seats"])
    assert seen > 0
    assert dkg_amd.seat_eval_shape(1024, 511, 16, 1024)["chunks"] > 1  # one seat of (1024, 511): 16 waves


def test_argument_errors():
    for args in ((0, 4, 1, 1, 0), (10, 4, 0, 1, 0), (10, 4, 1, 0, 0), (10, 4, 1, 11, 0), (10, 4, 1, 10, -1),
                 (100000, 70000, 1, 3, 1)):  # the last: more chunks than a launch grid holds
        with pytest.raises(DkgError) as e:
            dkg_amd.seat_eval_shape(*args)
        assert e.value.code == -1
    L = dkg_amd.lib()
    assert L.dkg_seat_eval_shape(10, 4, 1, 10, 0, None, None, None, None) == -1
    c = dkg_amd.seat_eval_shape(10, 4, 1, 10)["constants"]
    assert set(c) == {"launch_us", "op_latency_us", "lane_op_us", "serial_op_latency_us", "chunked_setup_us", "margin"}
    assert all(v > 0 for v in c.values())
