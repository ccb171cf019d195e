"""The proven-complaint rule on dealer shards, the parts that need no GPU: which rank owns a complaint
and how the ranks' verdict arrays merge (DKG_COMPLAINT_NOT_OWNED, an element-wise maximum), and the flag
words a rank sends beside its packed rows -- a Python model of dkg_shard_combine_proven_device, checked
against tests/finalise_ref.py (the reference's finalise as every party runs it) and against the PANIC rule
of dkg_ceremony_verify_fetched_proven.  tests/test_gpu_shard_proven.py holds the device to this model.
"""
import random

import pytest

import dkg_amd
from dkg_amd import ACCEPT, COMPLAINT_IGNORED, COMPLAINT_NO_PHASE3, COMPLAINT_NOT_OWNED, MISSING, REJECT, SELF
from dkg_amd._lib import FIN_INSUFFICIENT, FIN_OK, FIN_PANIC, FIN_PHASE4_ERROR
from dkg_amd.api import merge_verdicts, owning_rank, shard_range, shard_rows
from tests import finalise_ref as FR

FLAG_ROUND2, FLAG_ROUND4, FLAG_NO_PHASE3 = 1, 2, 4


# ---------------------------------------------------------------- ownership and the merge
def rank_view(n, ws, rank, accused, reference):
    """What rank `rank` of ws reports for a complaint list: the reference verdict of the complaints it owns
    (d0 < accused <= d1, 1-based accused), NOT_OWNED for the others."""
    d0, d1 = shard_range(n, ws, rank)
    return [v if d0 < i <= d1 else COMPLAINT_NOT_OWNED for i, v in zip(accused, reference)]


def test_not_owned_is_below_every_verdict():
    codes = [-1, 0, 1, 2, 3, COMPLAINT_IGNORED, COMPLAINT_NO_PHASE3]
    assert COMPLAINT_NOT_OWNED == -2 and all(COMPLAINT_NOT_OWNED < c for c in codes)


@pytest.mark.parametrize("ws", [1, 2, 3, 7, 8, 10])
def test_maximum_over_ranks_is_the_verdict_list(ws):
    """n = 10 over 1, 2, 3, 7 ranks and over more ranks than n / 2 (8, 10: some ranks own one dealer or none
    at ws > n): every complaint is owned by exactly one rank, in any order and with duplicates, and the
    element-wise maximum of the ranks' arrays is the reference list."""
    n = 10
    rng = random.Random(ws)
    accused = [rng.randrange(1, n + 1) for _ in range(40)] + [1, n, 1, n]
    reference = [rng.choice([-1, 0, 1, 2, 3, COMPLAINT_IGNORED, COMPLAINT_NO_PHASE3]) for _ in accused]
    views = [rank_view(n, ws, r, accused, reference) for r in range(ws)]
    for c, i in enumerate(accused):
        owners = [r for r in range(ws) if views[r][c] != COMPLAINT_NOT_OWNED]
        assert owners == [owning_rank(n, ws, i - 1)], (c, i)
    assert merge_verdicts(views) == reference
    assert merge_verdicts([[] for _ in range(ws)]) == []
    with pytest.raises(ValueError):  # a list that some rank did not see whole: nobody owns complaint 0
        merge_verdicts([[COMPLAINT_NOT_OWNED] + v[1:] for v in views])


def test_ranks_without_dealers():
    """ws = 3 at n = 4: dkg_shard_range leaves nobody empty there (1, 1, 2); ws > n does."""
    assert [shard_range(4, 3, r) for r in range(3)] == [(0, 1), (1, 2), (2, 4)]
    assert shard_range(2, 3, 0) == (0, 0) and shard_rows(2, 3) == 1
    assert rank_view(2, 3, 0, [1, 2], [0, 3]) == [COMPLAINT_NOT_OWNED] * 2


# ---------------------------------------------------------------- the send block and the verdict merge over gloo
def _free_port():
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _layout_main(rank, ws, port, errq):
    import torch
    import torch.distributed as dist

    from dkg_amd.distributed import ShardedCeremony

    try:
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=ws)
        n, t = 10, 4
        sc = ShardedCeremony(None, dist, n, t, torch.device("cpu"))
        R, W1 = sc.R, sc.W1
        S = 2 * 4 * R * W1 + 32 * R + 32 * n
        assert sc.exchange_bytes() == sc.exchange_bytes(proven=False) == S
        assert sc.exchange_bytes(proven=True) == S + 4 * R + 4 * n
        sc._proven_init()
        assert sc.send.numel() == S and sc.p_send.numel() == S + 4 * R + 4 * n  # the existing block is untouched
        mark = lambda r, k: 16 * (r + 1) + k  # noqa: E731
        sc._pack = lambda dec, out: out.fill_(mark(rank, 1 if dec is sc.dec2 else 2))
        sc.pA0.fill_(mark(rank, 3))
        sc.ppart.fill_(mark(rank, 4))
        sc.pflags.fill_(mark(rank, 5))
        sc.pdis.fill_(mark(rank, 6))
        g2, g4, gA0, gpart, gfl, gdis = sc.exchange_proven()
        for r in range(ws):  # ONE gather delivered every rank's six parts, each to its own array
            assert g2.view(ws, R * W1)[r].tolist() == [mark(r, 1)] * (R * W1)
            assert g4.view(ws, R * W1)[r].tolist() == [mark(r, 2)] * (R * W1)
            assert gA0.view(ws, 32 * R)[r].tolist() == [mark(r, 3)] * (32 * R)
            assert gpart.view(ws, 32 * n)[r].tolist() == [mark(r, 4)] * (32 * n)
            assert gfl.view(ws, R)[r].tolist() == [mark(r, 5)] * R
            assert gdis.view(ws, n)[r].tolist() == [mark(r, 6)] * n
        accused = [3, 10, 1, 6, 6, 5, 9]
        reference = [0, 2, COMPLAINT_IGNORED, -1, 3, COMPLAINT_NO_PHASE3, 1]
        assert sc._merge_verdicts(rank_view(n, ws, rank, accused, reference)) == reference
        assert sc._merge_verdicts([]) == []
        with pytest.raises(ValueError):
            ShardedCeremony(None, dist, n, t, torch.device("cpu"), packed=False).run_verify_proven(0, 0, 0, 0, [], [],
                                                                                                  b"", b"")
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:  # report to the parent; a hung peer is cut by the join timeout
        errq.put(f"rank {rank}: {type(e).__name__}: {e}")
        raise


def test_proven_send_block_over_gloo():
    """The proven runs' send block -- the packed block, then [R] flag words and [n] dissent words -- goes
    through ONE all_gather_into_tensor, and one all_reduce(MAX) merges the ranks' verdict arrays (three gloo
    processes on CPU tensors, no GPU)."""
    import torch.multiprocessing as mp

    ws = 3
    ctx = mp.get_context("spawn")
    errq = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_layout_main, args=(r, ws, port, errq)) for r in range(ws)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=120)
    alive = [p for p in procs if p.is_alive()]
    for p in alive:
        p.kill()
    errs = []
    while not errq.empty():
        errs.append(errq.get())
    assert not alive, "rank hung"
    assert not errs, errs
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]


# ---------------------------------------------------------------- the flag-word model
def flag_outcome(n, t, dec2, dec4, flags, full):
    """dkg_shard_combine_proven_device restated: dec2 / dec4 the ranks' raw rows [n][n] (REJECT / ACCEPT,
    SELF on the diagonal, whole rows of MISSING in dec2), flags [n] the ranks' flag words.  Returns the
    common outcome as a dict (dec4 with the SKIPPED rows applied)."""
    missing = [MISSING in dec2[i] for i in range(n)]
    if full:
        qualified = [int(not missing[i] and not flags[i] & FLAG_ROUND2) for i in range(n)]
    else:
        qualified = [int(not missing[i] and REJECT not in dec2[i]) for i in range(n)]
    complaints2 = [sum(dec2[i][j] == REJECT for i in range(n)) for j in range(n)]
    r2_error = [int(c > t) for c in complaints2]
    reconstruct = [int(qualified[i] and bool(flags[i] & FLAG_ROUND4)) for i in range(n)]
    r4_error = [int(1 + sum(qualified[i] and dec4[i][j] == ACCEPT for i in range(n)) < t + 1) for j in range(n)]
    out4 = [[3 if not qualified[i] and j != i else dec4[i][j] for j in range(n)] for i in range(n)]
    phase4_error = int(sum(qualified) - sum(reconstruct) <= t)
    status, index = FIN_OK, -1
    if phase4_error:
        status = FIN_PHASE4_ERROR
    else:
        disclosing = [qualified[j] and not reconstruct[j] and not r2_error[j] and not r4_error[j] for j in range(n)]
        for i in range(n):
            if reconstruct[i] and sum(disclosing) < t:
                status, index = FIN_INSUFFICIENT, i
            elif not reconstruct[i] and qualified[i] and flags[i] & FLAG_NO_PHASE3:
                status, index = FIN_PANIC, i
            if status != FIN_OK:
                break
    return dict(qualified=qualified, complaints2=complaints2, r2_error=r2_error, reconstruct=reconstruct,
                r4_error=r4_error, dec4=out4, phase4_error=phase4_error, n_qualified=sum(qualified),
                finalise_status=status, recovery_index=index)


def honest_rows(n):
    return [[SELF if i == j else ACCEPT for j in range(n)] for i in range(n)]


FR_STATUS = {"OK": FIN_OK, "PHASE4_ERROR": FIN_PHASE4_ERROR, "INSUFFICIENT": FIN_INSUFFICIENT}


def fr_common(n, t, o):
    """The finalising parties' (status, index) by tests/finalise_ref.py, for outcomes in which every dealer
    is qualified: every party that is not reconstructed and has no r2 / r4 error reports the same.  (With a
    disqualified dealer party_finalise models the other parties' expect() at committee.rs:791-794, a state
    the common outcome does not carry, under the rejection rule either.)"""
    assert all(o["qualified"])
    A0 = [FR.g_mul(100 + i) for i in range(n)]
    return {FR.party_finalise(p, n, t, o["qualified"], o["reconstruct"], A0, lambda i, j: 7 * i + j + 1,
                              r2_error=o["r2_error"], r4_error=o["r4_error"])[:2]
            for p in range(n) if not o["reconstruct"][p] and not o["r2_error"][p] and not o["r4_error"][p]}


def test_flag_model_ok_and_reconstruction():
    n, t = 10, 4
    o = flag_outcome(n, t, honest_rows(n), honest_rows(n), [0] * n, True)
    assert (o["finalise_status"], o["recovery_index"], o["n_qualified"], o["phase4_error"]) == (FIN_OK, -1, n, 0)
    assert fr_common(n, t, o) == {("OK", -1)}
    flags = [0] * n
    flags[5] = FLAG_ROUND4
    o = flag_outcome(n, t, honest_rows(n), honest_rows(n), flags, True)
    assert o["reconstruct"] == [int(i == 5) for i in range(n)] and o["finalise_status"] == FIN_OK
    assert fr_common(n, t, o) == {("OK", -1)}


def test_flag_model_a_rejection_alone_decides_nothing():
    """Full mode: a REJECT without flag bit 0 keeps the dealer (the swapped-share dealer); with it the dealer
    leaves, its round-4 row is SKIPPED and a round-4 flag against it reconstructs nobody."""
    n, t = 10, 4
    dec2 = honest_rows(n)
    dec2[3][7] = REJECT
    o = flag_outcome(n, t, dec2, honest_rows(n), [0] * n, True)
    assert o["qualified"] == [1] * n and o["complaints2"][7] == 1
    assert flag_outcome(n, t, dec2, honest_rows(n), [0] * n, False)["qualified"] == [int(i != 3) for i in range(n)]
    flags = [0] * n
    flags[3] = FLAG_ROUND2 | FLAG_ROUND4
    o = flag_outcome(n, t, dec2, honest_rows(n), flags, True)
    assert o["qualified"] == [int(i != 3) for i in range(n)] and o["reconstruct"] == [0] * n
    assert o["dec4"][3] == [SELF if j == 3 else 3 for j in range(n)]
    dec2[6] = [SELF if j == 6 else MISSING for j in range(n)]
    assert flag_outcome(n, t, dec2, honest_rows(n), [0] * n, True)["qualified"][6] == 0


def test_flag_model_phase4_error_and_insufficient():
    n, t = 10, 4
    flags = [FLAG_ROUND4 if i in (0, 2, 4, 5, 7, 9) else 0 for i in range(n)]
    o = flag_outcome(n, t, honest_rows(n), honest_rows(n), flags, True)
    assert (o["phase4_error"], o["finalise_status"], o["recovery_index"]) == (1, FIN_PHASE4_ERROR, -1)
    assert fr_common(n, t, o) == {("PHASE4_ERROR", -1)}
    # n = 16, t = 3: dealers 2 and 9 reconstructed, and all but two of the final parties saw more than t
    # complaints (an r2 error: they never disclose): 2 < t points, INSUFFICIENT at the FIRST such dealer
    n, t = 16, 3
    dec2 = honest_rows(n)
    for j in range(n):
        if j not in (0, 1):
            for i in (11, 12, 13, 14, 15):
                if i != j:
                    dec2[i][j] = REJECT
    flags = [FLAG_ROUND4 if i in (2, 9) else 0 for i in range(n)]
    o = flag_outcome(n, t, dec2, honest_rows(n), flags, True)
    assert o["qualified"] == [1] * n and o["r2_error"] == [int(j > 1) for j in range(n)]
    assert (o["finalise_status"], o["recovery_index"]) == (FIN_INSUFFICIENT, 2)
    assert fr_common(n, t, o) == {("INSUFFICIENT", 2)}


def test_flag_model_panic():
    """A qualified dealer without a usable phase-3 broadcast that nobody complained about: PANIC at it,
    before a later reconstructed dealer is reached; one complaint (bit 1) turns it into a reconstruction."""
    n, t = 10, 4
    flags = [0] * n
    flags[2] = FLAG_NO_PHASE3
    flags[5] = FLAG_ROUND4
    o = flag_outcome(n, t, honest_rows(n), honest_rows(n), flags, False)
    assert (o["finalise_status"], o["recovery_index"]) == (FIN_PANIC, 2)
    flags[2] |= FLAG_ROUND4
    o = flag_outcome(n, t, honest_rows(n), honest_rows(n), flags, False)
    assert o["reconstruct"] == [int(i in (2, 5)) for i in range(n)]
    assert (o["finalise_status"], o["recovery_index"]) == (FIN_OK, -1)
    assert fr_common(n, t, o) == {("OK", -1)}
    flags[2] = FLAG_NO_PHASE3 | FLAG_ROUND2  # disqualified in round 2: not a panic of the common outcome
    o = flag_outcome(n, t, honest_rows(n), honest_rows(n), flags, True)
    assert (o["finalise_status"], o["recovery_index"]) == (FIN_OK, -1)
