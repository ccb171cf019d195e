"""The proven-complaint rule of the dealer-sharded path across processes: ShardedCeremony.run_verify_proven /
run_verify_full_proven + the sharded proven entry points + ONE all-gather of the grown send block + one
all_reduce(MAX) per verdict list + dkg_shard_combine_proven_device, in 2 and 3 spawned ranks that share
GPU 0 over gloo and in one rank over RCCL (tests/dist_worker_proven.py).  Every combined output equals the
single-context call's on the same inputs."""
import json
import os
import socket
import subprocess
import sys

import pytest

import dkg_amd
from dkg_amd import packed_row_words, shard_rows
from dkg_amd._lib import FIN_INSUFFICIENT, FIN_PANIC, FIN_PHASE4_ERROR
from tests.test_gpu import CK
from tests.test_gpu_batch_proven import faulted_ceremony
from tests.test_gpu_shard_proven import (FULL_DIST, PLAIN_DIST, full_scenarios, plain_scenarios, single_full,
                                         single_plain)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _spawn(ws, backend, args, timeout=100):
    port = _free_port()
    procs = []
    for r in range(ws):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(ws), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), DKG_DIST_BACKEND=backend)
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dist_worker_proven.py")] + args,
                                      env=env))
    try:
        rcs = [p.wait(timeout=timeout) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert rcs == [0] * ws, rcs


def expected(p, full):
    r = p.result
    d = {"dec2": "".join(str(v) for v in r.dec2), "dec4": "".join(str(v) for v in r.dec4),
         "qualified": list(r.qualified), "reconstruct": list(r.reconstruct), "complaints2": list(r.complaints2),
         "r4_error": list(r.r4_error), "r2_error": list(r.r2_error), "phase4_error": bool(r.phase4_error),
         "final_share": r.final_share.hex(), "public_share": r.public_share.hex(),
         "mpk": None if r.mpk == bytes(32) else r.mpk.hex(), "verdict4": p.verdict4,
         "finalise_status": p.finalise_status, "recovery_index": p.recovery_index,
         "verdict": p.verdict if full else None, "dissent": p.dissent if full else None}
    return d


@pytest.fixture(scope="module")
def references(golden):
    """The single-context calls on the worker's scenarios."""
    be = dkg_amd.Backend(0)
    try:
        cer = faulted_ceremony(golden)
        cer["s"], cer["s_prime"] = cer.pop("shares")
        want = {}
        for name in FULL_DIST:
            c2, c4, f3 = full_scenarios(cer)[name]
            want["full:" + name] = expected(single_full(be, cer, c2, c4, f3), True)
        for name in PLAIN_DIST:
            pc, c4, f1, f3 = plain_scenarios(be, golden)[name]
            want["plain:" + name] = expected(single_plain(be, pc, c4, f1, f3), False)
        be.env_init(cer["t"], cer["n"], CK)
        rej = be.ceremony_verify_full(cer["E"], cer["A"], cer["e1"], cer["ct"], cer["sk"], cer["n"], cer["t"])
        want["rejection"] = {"qualified": list(rej.qualified), "reconstruct": list(rej.reconstruct),
                             "mpk": rej.mpk.hex(), "dec4": "".join(str(v) for v in rej.dec4)}
    finally:
        be.close()
    assert want["full:no_phase3_silent"]["finalise_status"] == FIN_PANIC
    assert want["plain:no_phase3_silent"]["finalise_status"] == FIN_PANIC
    assert want["plain:insufficient"]["finalise_status"] == FIN_INSUFFICIENT
    assert want["plain:phase4"]["finalise_status"] == FIN_PHASE4_ERROR
    return want


def test_rules_alternate_on_one_object(tmp_path, references):
    """Three ranks over gloo (dealers 3, 3, 4): rejection-rule and proven runs alternating on ONE
    ShardedCeremony -- one _finish and one block-splitting routine serve both -- each equal to the same run
    on an object of its own, with exchange_bytes() reporting the kind of the run just made."""
    out = tmp_path / "dist_mixed.json"
    _spawn(3, "gloo", [str(out), "mixed"])
    runs = json.loads(out.read_text())["mixed"]
    assert [k for k, _, _ in runs] == ["rejection_full", "proven_full", "rejection_full", "rejection_plain",
                                       "proven_plain", "rejection_plain", "proven_full"]
    n = 10
    R = shard_rows(n, 3)
    S = 2 * 4 * R * packed_row_words(n) + 32 * R + 32 * n
    for kind, one, fresh in runs:
        assert one == fresh, kind
        proven = kind.startswith("proven")
        assert one["exchange_bytes"] == (S + 4 * R + 4 * n if proven else S) and one["plain_bytes"] == S, kind
        assert (one["verdict4"] is not None) == proven and (one["verdict"] is not None) == (kind == "proven_full")
    for k, v in references["full:honest"].items():
        assert runs[1][1][k] == v and runs[6][1][k] == v, k
    for k, v in references["rejection"].items():
        assert runs[0][1][k] == v and runs[2][1][k] == v, k
    assert runs[3][1] == runs[5][1]


@pytest.mark.parametrize("ws,backend", [(2, "gloo"), (3, "gloo"), (1, "nccl")])
def test_sharded_proven_processes(tmp_path, references, ws, backend):
    out = tmp_path / "dist_proven.json"
    _spawn(ws, backend, [str(out)])
    res = json.loads(out.read_text())
    assert sorted(res) == sorted(list(references) + ["raw_rows"])
    assert res["raw_rows"] == "ValueError"
    for key, want in references.items():
        got = res[key]
        for k, v in want.items():
            assert got[k] == v, (key, k)
        n = len(want["qualified"])
        R = shard_rows(n, ws)
        S = 2 * 4 * R * packed_row_words(n) + 32 * R + 32 * n
        if key == "rejection":
            assert got["exchange_bytes"] == S  # the existing block, after proven runs on the same object
        else:
            assert (got["plain_bytes"], got["exchange_bytes"]) == (S, S + 4 * R + 4 * n), key
