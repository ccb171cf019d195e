"""The phase-4 broadcast intake (dkg_amd.broadcast.intake_phase4): MembersFetchedState4::from_broadcast and
FetchedMisbehaviourComplaints::from_broadcasts_4 (committee.rs:964-993, 1027-1070) committee-wide,
flattened for Backend.complaints3_verify.  CPU only."""
import pytest

from dkg_amd.broadcast import BroadcastPhase4, MisbehavingPartiesRound3, intake_phase4


def _mp(accused, tag):
    return MisbehavingPartiesRound3(accused, bytes([tag]) * 32, bytes([tag + 1]) * 32)


def test_round_trip_and_positions():
    n = 5
    msgs = [BroadcastPhase4([_mp(3, 10), _mp(4, 20)]), None, BroadcastPhase4([]), BroadcastPhase4([_mp(1, 30)]), None]
    wire = [None if m is None else m.to_bytes() for m in msgs]
    back = [None if w is None else BroadcastPhase4.from_bytes(w) for w in wire]
    assert back == msgs
    accuser, accused, share, randomness = intake_phase4(n, back)
    # sender index = position + 1; an absent broadcast (None) is dropped, an empty one contributes nothing
    assert accuser == [1, 1, 4]
    assert accused == [3, 4, 1]
    assert share == bytes([10]) * 32 + bytes([20]) * 32 + bytes([30]) * 32
    assert randomness == bytes([11]) * 32 + bytes([21]) * 32 + bytes([31]) * 32


def test_duplicates_and_self_accusations_pass_through():
    m = BroadcastPhase4([_mp(2, 1), _mp(2, 3), _mp(1, 5)])
    assert intake_phase4(2, [m, None])[:2] == ([1, 1, 1], [2, 2, 1])


def test_nothing_broadcast():
    assert intake_phase4(3, [None, None, None]) == ([], [], b"", b"")


def test_shape_errors():
    with pytest.raises(ValueError):
        intake_phase4(3, [None, None])
    with pytest.raises(ValueError):
        intake_phase4(3, [None, None, None, None])
    for bad in (0, 4):
        with pytest.raises(ValueError):
            intake_phase4(3, [BroadcastPhase4([_mp(bad, 1)]), None, None])
    with pytest.raises(ValueError):
        intake_phase4(2, [BroadcastPhase4([MisbehavingPartiesRound3(2, b"\x01" * 31, b"\x07" * 32)]), None])
    with pytest.raises(ValueError):
        BroadcastPhase4.from_bytes(BroadcastPhase4([_mp(1, 1)]).to_bytes()[:-1])
