"""The phase-2 broadcast intake (dkg_amd.broadcast.intake_phase2): MembersFetchedState2::from_broadcast
(committee.rs:878-910) committee-wide, flattened for Backend.complaints_verify.  CPU only."""
import pytest

from dkg_amd.broadcast import BroadcastPhase2, MisbehavingPartiesRound1, intake_phase2


def _mp(accused, tag):
    return MisbehavingPartiesRound1(accused, 3, bytes([tag]) * 128, bytes([tag + 1]) * 192)


def test_round_trip_and_positions():
    n = 5
    msgs = [BroadcastPhase2([_mp(3, 10), _mp(4, 20)]), None, BroadcastPhase2([]), BroadcastPhase2([_mp(1, 30)]), None]
    wire = [None if m is None else m.to_bytes() for m in msgs]
    back = [None if w is None else BroadcastPhase2.from_bytes(w) for w in wire]
    assert back == msgs
    accuser, accused, proofs = intake_phase2(n, back)
    # sender index = position + 1; an absent broadcast (None) is dropped, an empty one contributes nothing
    assert accuser == [1, 1, 4]
    assert accused == [3, 4, 1]
    assert proofs == bytes([11]) * 192 + bytes([21]) * 192 + bytes([31]) * 192


def test_ciphertext_copy_is_ignored():
    """verify reads the accused's own phase-1 broadcast (broadcast.rs:57), not the complaint's copy."""
    a = intake_phase2(2, [BroadcastPhase2([MisbehavingPartiesRound1(2, 3, b"\x01" * 128, b"\x07" * 192)]), None])
    b = intake_phase2(2, [BroadcastPhase2([MisbehavingPartiesRound1(2, 9, b"\x02" * 128, b"\x07" * 192)]), None])
    assert a == b == ([1], [2], b"\x07" * 192)


def test_duplicates_and_self_accusations_pass_through():
    m = BroadcastPhase2([_mp(2, 1), _mp(2, 3), _mp(1, 5)])
    assert intake_phase2(2, [m, None])[:2] == ([1, 1, 1], [2, 2, 1])


def test_nothing_broadcast():
    assert intake_phase2(3, [None, None, None]) == ([], [], b"")


def test_shape_errors():
    with pytest.raises(ValueError):
        intake_phase2(3, [None, None])
    for bad in (0, 4):
        with pytest.raises(ValueError):
            intake_phase2(3, [BroadcastPhase2([_mp(bad, 1)]), None, None])
    with pytest.raises(ValueError):
        intake_phase2(2, [BroadcastPhase2([MisbehavingPartiesRound1(2, 3, b"\x01" * 128, b"\x07" * 191)]), None])
