"""Full (encrypted-share) mode of the dealer-sharded path across processes: ShardedCeremony.run_full /
run_verify_full + dkg_ceremony_shard_full_device / _shard_verify_full_device + the unchanged all-gathers,
combine, reconstruction exchange and finalise, in 2 and 3 spawned ranks that share GPU 0 over gloo and in
one rank over RCCL (tests/dist_worker_full.py).  Every combined output equals the libsodium full-mode
fixtures, the tampered ciphertexts included."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = ["full_n4_t1.json", "full_n10_t4.json", "full_faults_n10_t4.json"]


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
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dist_worker_full.py")] + args,
                                      env=env))
    try:
        rcs = [p.wait(timeout=timeout) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert rcs == [0] * ws, rcs


@pytest.mark.parametrize("ws,backend", [(2, "gloo"), (3, "gloo"), (1, "nccl")])
def test_sharded_full_ceremony_processes(tmp_path, golden, ws, backend):
    out = tmp_path / "dist_full.json"
    _spawn(ws, backend, [str(out)])
    res = json.loads(out.read_text())
    assert sorted(res) == sorted(["verify:" + f for f in FULL] + ["run:" + f for f in FULL[:2]])
    for key, got in res.items():
        c = golden(key.split(":", 1)[1])
        for k in ("dec2", "dec4", "qualified", "reconstruct", "complaints2", "final_share", "public_share"):
            assert got[k] == c[k], (key, k)
        assert got["r4_error"] == [int(x) for x in c["r4_error"]], key
        assert got["phase4_error"] == c["phase4_error"], key
        if c["phase4_error"] or c["mpk"] == "00" * 32:
            assert got["mpk"] is None, key
        else:
            assert got["mpk"] == c["mpk"], key
