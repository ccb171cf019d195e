"""dkg_seat_pack (host only): how one operator's seats (ceremony, party index) share the waves of
k_seat_horner.  Seats are grouped by x = j + 1 ascending, keep caller order inside a group and fill waves
of per_wave slots; a wave never holds two x; a seat with n > 64 takes `tiles` consecutive waves.  A plain
Python model of the lane map (lane -> seat, dealer, live) is run against that definition."""
import ctypes
import random
from collections import Counter

import pytest

import dkg_amd
from dkg_amd import DkgError

SHAPES = {2: (2, 32, 1), 3: (4, 16, 1), 10: (16, 4, 1), 16: (16, 4, 1), 32: (32, 2, 1), 33: (64, 1, 1),
          64: (64, 1, 1), 70: (64, 1, 2), 130: (64, 1, 3)}  # n: (W, per_wave, tiles)


def seat_lists(n):
    rng = random.Random(7000 + n)
    yield [0]
    yield [n - 1]
    yield [n - 1, 0, n - 1, 0]                          # two groups, interleaved in caller order
    yield [n // 2] * 131                                # one group over many waves, the last partly filled
    yield [3 % n, 3 % n, 3 % n, 3 % n, 3 % n, 7 % n, 7 % n, 1 % n, n - 1]
    yield list(range(n)) * 3                            # every x, three seats each
    for S in (1, 5, 64, 257, 1000):
        yield [rng.randrange(n) for _ in range(S)]
    yield [min(n - 1, int(rng.expovariate(0.3))) for _ in range(500)]  # a few crowded groups


@pytest.mark.parametrize("n", sorted(SHAPES))
def test_shape(n):
    p = dkg_amd.seat_pack(n, [0])
    assert (p["width"], p["per_wave"], p["tiles"]) == SHAPES[n]
    assert p["width"] * p["per_wave"] == 64 and (p["width"] >= n or p["width"] == 64)
    assert p["width"] == 64 or p["width"] < 2 * n       # the power of two >= n, not a larger one


@pytest.mark.parametrize("n", sorted(SHAPES))
def test_placement(n):
    W, per, tiles = SHAPES[n]
    for js in seat_lists(n):
        p = dkg_amd.seat_pack(n, js)
        S = len(js)
        assert (p["width"], p["per_wave"], p["tiles"]) == (W, per, tiles)
        counts = Counter(js)
        assert p["waves"] == sum(-(-c // per) * tiles for c in counts.values())
        # every seat once: the (wave, slot) cells are distinct, inside the launch, tile-aligned runs
        cells = {}
        for q in range(S):
            w0, sl = p["wave_of"][q], p["slot_of"][q]
            assert sl < per and w0 + tiles <= p["waves"]
            for tile in range(tiles):
                assert (w0 + tile, sl) not in cells
                cells[(w0 + tile, sl)] = (q, tile)
        assert len(cells) == S * tiles
        # one x per wave; groups in ascending x; caller order inside a group, filled densely
        wave_x = {}
        for (w, _), (q, _) in cells.items():
            assert wave_x.setdefault(w, js[q]) == js[q]
        assert sorted(wave_x) == list(range(p["waves"]))  # no wave without a seat
        xs_by_wave = [wave_x[w] for w in range(p["waves"])]
        assert xs_by_wave == sorted(xs_by_wave)
        for x in counts:
            members = [q for q in range(S) if js[q] == x]
            first = min(p["wave_of"][q] for q in members)
            for r, q in enumerate(members):
                assert (p["wave_of"][q], p["slot_of"][q]) == (first + (r // per) * tiles, r % per)


def lane_model(n, js, p):
    """{(wave, lane): (seat, dealer)} of the live lanes, from the placement alone: lane slot * W + i of wave
    wave_of[q] + tile is dealer tile * 64 + i of seat q, live where that is < n."""
    W = p["width"]
    live = {}
    for q in range(len(js)):
        for tile in range(p["tiles"]):
            for i in range(W):
                d = tile * 64 + i
                if d < n:
                    key = (p["wave_of"][q] + tile, p["slot_of"][q] * W + i)
                    assert key not in live
                    live[key] = (q, d)
    return live


@pytest.mark.parametrize("n", sorted(SHAPES))
def test_lane_map(n):
    for js in seat_lists(n):
        p = dkg_amd.seat_pack(n, js)
        live = lane_model(n, js, p)
        # every (seat, dealer) pair is evaluated by exactly one lane, and every lane is in range
        assert sorted(live.values()) == [(q, d) for q in range(len(js)) for d in range(n)]
        assert all(w < p["waves"] and lane < 64 for w, lane in live)
        # the lanes of one slot are consecutive dealers (contiguous table columns)
        for (w, lane), (q, d) in live.items():
            if lane % p["width"]:
                assert live[(w, lane - 1)] == (q, d - 1)
        # dead lanes: i >= n inside a slot, empty slots, the ragged last tile
        dead = 64 * p["waves"] - len(live)
        per, tiles, W = p["per_wave"], p["tiles"], p["width"]
        empty_slots = p["waves"] * per - len(js) * tiles
        assert dead == empty_slots * W + len(js) * (tiles * W - n)


def test_arguments():
    L = dkg_amd.lib()
    u32 = ctypes.c_uint32
    v = [u32(9) for _ in range(4)]
    refs = [ctypes.byref(x) for x in v]
    js = (u32 * 3)(0, 1, 2)
    wave_of, slot_of = (u32 * 3)(), (u32 * 3)()

    def call(n, S, js_, outs=None, wo=wave_of, so=slot_of):
        o = refs if outs is None else outs
        return L.dkg_seat_pack(n, S, js_, o[0], o[1], o[2], wo, so, o[3])

    assert call(10, 3, js) == 0 and v[3].value == 3   # three x, three waves
    assert call(0, 3, js) == -1                        # n == 0
    assert call(0, 0, None) == -1
    assert call(3, 3, js) == 0 and call(2, 3, js) == -1  # js[p] >= n
    assert call(10, 3, None) == -1
    for k in range(4):                                 # a NULL output with S > 0
        outs = list(refs)
        outs[k] = None
        assert call(10, 3, js, outs) == -1
    assert call(10, 3, js, wo=None) == -1 and call(10, 3, js, so=None) == -1
    v[3].value = 9                                     # S == 0: DKG_OK, *waves = 0, the lists untouched
    assert call(10, 0, None, wo=None, so=None) == 0
    assert [x.value for x in v] == [16, 4, 1, 0]
    assert dkg_amd.seat_pack(10, []) == {"width": 16, "per_wave": 4, "tiles": 1, "wave_of": [], "slot_of": [],
                                         "waves": 0}
    with pytest.raises(DkgError):
        dkg_amd.seat_pack(10, [10])
    with pytest.raises(DkgError):
        dkg_amd.seat_pack(0, [])
