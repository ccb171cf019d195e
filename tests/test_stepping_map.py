"""CPU checks of the stepping's banded lane map (dkg_amd/csrc/step_map.h through
dkg_stepping_lane_map): over every workgroup shape the GPU cases of test_gpu_stepping_bands.py
reach, and every other shape of equal segments that fills a workgroup, the map is a bijection of
lanes onto (segment, position), the neighbour lane holds the next position of the same segment,
wave w's lowest position is wB, and the LDS reads of a 32-lane group fall on distinct banks.
Shapes that must keep the contiguous map (a lone segment, a ragged last piece, idle lanes) report
band 0."""
import ctypes

import pytest

from dkg_amd import _lib

# (lanes, segment length P, segments per slot): P = 128 x 2 (the n = 1024 headline's pieces),
# P = 64 x 4 per piece and as the four pieces of one column, P = 128 x 4 in 512 lanes, P = 32 x 8
# (n = 70, t = 63, U = 2: per piece, and two pieces per column slot), P = 96 x 2 in 192 lanes
BANDED = [(256, 128, 1), (256, 64, 1), (256, 64, 4), (512, 128, 1), (512, 128, 4), (256, 32, 1), (256, 32, 2),
          (192, 96, 1), (512, 256, 2), (256, 4, 1), (512, 8, 1)]


def lane_map(lanes, P, nseg, last):
    L = _lib.lib()
    out = (ctypes.c_int * 3)()
    rows, band = [], None
    for lane in range(lanes):
        b = L.dkg_stepping_lane_map(lanes, P, nseg, last, lane, out)
        assert band in (None, b)
        band = b
        rows.append(tuple(out) if b > 0 else None)
    return band, rows


@pytest.mark.parametrize("lanes,P,nseg", BANDED)
def test_banded_map(lanes, P, nseg):
    S = lanes // P
    B, rows = lane_map(lanes, P, nseg, P)
    assert B == 64 // S
    # bijection of lanes onto (segment, position)
    assert sorted((s, q) for s, q, _ in rows) == [(s, q) for s in range(S) for q in range(P)]
    for lane, (s, q, nxt) in enumerate(rows):
        w = lane // 64
        assert w * B <= q < (w + 1) * B  # wave w holds the band [wB, (w+1)B) of every segment
        assert 0 <= nxt < lanes and rows[nxt][0] == s
        assert rows[nxt][1] == (q + 1 if q + 1 < P else 0)  # past the top: a column of the same segment
    for w in range(lanes // 64):
        assert min(rows[l][1] for l in range(64 * w, 64 * w + 64)) == w * B
    # ds_read_b32 is serviced in lane groups of 32 with bank = word mod 32: the addend reads of the
    # lanes that add (every position but a segment's top) stay on distinct banks
    for g in range(lanes // 32):
        banks = [rows[l][2] % 32 for l in range(32 * g, 32 * g + 32) if rows[l][1] + 1 < P]
        assert len(banks) == len(set(banks))


@pytest.mark.parametrize("lanes,P,nseg,last", [
    (512, 512, 1, 512),   # config E: one segment per workgroup
    (256, 101, 1, 101),   # slots that leave lanes idle
    (256, 101, 2, 100),   # ragged last piece
    (256, 128, 2, 100),
    (384, 128, 1, 128),   # three segments do not divide a wave
    (256, 64, 3, 64),     # slots of three segments do not fill four
])
def test_contiguous_shapes_keep_their_map(lanes, P, nseg, last):
    band, _ = lane_map(lanes, P, nseg, last)
    assert band == 0


def test_bad_input():
    L = _lib.lib()
    out = (ctypes.c_int * 3)()
    assert L.dkg_stepping_lane_map(256, 128, 1, 128, 256, out) == -1
    assert L.dkg_stepping_lane_map(100, 50, 1, 50, 0, out) == -1
    assert L.dkg_stepping_lane_map(256, 128, 1, 128, 0, None) == -1


def test_split_model_keeps_four_pieces():
    """The headline shapes keep U = 4 with the dead-wave discount in the stepping's price."""
    L = _lib.lib()
    for n in (1024, 4096):
        t = n // 2 - 1
        ms = {U: L.dkg_split_model_ms(n, n, t, U) for U in range(1, 9)}
        assert min(ms, key=ms.get) == 4, ms
