"""One rank of tests/test_gpu_dist_proven.py (not a test module): the proven-complaint rule of the
dealer-sharded ceremony end to end through dkg_amd.distributed.ShardedCeremony.run_verify_full_proven /
run_verify_proven on GPU 0 -- ranks sharing the GPU over gloo, or one rank over RCCL
(DKG_DIST_BACKEND=nccl), as tests/dist_worker.py.  Every rank passes the WHOLE complaint lists and
uploads only its dealers' rows.  Rank 0 writes the combined outputs as JSON to argv[1], keyed
"full:<scenario>" / "plain:<scenario>" (tests/test_gpu_shard_proven.py full_scenarios, plain_scenarios); with
argv[2] = "mixed", the runs of mixed() under "mixed" instead."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libdkg_amd.so: its HIP runtime must be torch's)
import torch.distributed as dist  # noqa: E402

import dkg_amd  # noqa: E402
from dkg_amd.distributed import ShardedCeremony, dealer_range  # noqa: E402
from tests.dist_worker import golden, summary  # noqa: E402
from tests.test_gpu_batch_proven import faulted_ceremony  # noqa: E402
from tests.test_gpu_shard_proven import (FULL_DIST, PLAIN_DIST, full_scenarios, lists2, lists4,  # noqa: E402
                                         plain_scenarios)


def proven_summary(res, sc):
    d = summary(res)
    d.update(verdict=res.verdict, verdict4=res.verdict4, dissent=res.dissent, finalise_status=res.finalise_status,
             recovery_index=res.recovery_index, r2_error=[int(x) for x in res.decisions.r2_error],
             exchange_bytes=sc.exchange_bytes(), plain_bytes=sc.exchange_bytes(proven=False))
    return d


def mixed(be, dev, rank, ws, put):
    """Rejection-rule and proven runs alternating on ONE ShardedCeremony, each also on an object of its own
    (argv[2] = "mixed"): [[kind, summary on the shared object, summary on the fresh one]]."""
    cer = faulted_ceremony(golden)
    cer["s"], cer["s_prime"] = cer.pop("shares")
    n, t = cer["n"], cer["t"]
    N = t + 1
    be.env_init(t, n)
    d0, d1 = dealer_range(rank, ws, n)
    ins = [put(cer[k][w * d0:w * d1]) for k, w in (("E", 32 * N), ("A", 32 * N), ("e1", 64 * n), ("ct", 64 * n),
                                                   ("s", 32 * n), ("s_prime", 32 * n))]  # alive until the return
    E, A, e1, ct, s, sp = (x.data_ptr() for x in ins)
    c2, c4 = lists2(cer["c2"]), lists4(cer["c4"])
    runs = {"rejection_full": lambda sc: sc.run_verify_full(E, A, e1, ct, cer["sk"]),
            "proven_full": lambda sc: sc.run_verify_full_proven(E, A, e1, ct, cer["sk"], cer["pk"], *c2, *c4),
            "rejection_plain": lambda sc: sc.run_verify(E, A, s, sp),
            "proven_plain": lambda sc: sc.run_verify_proven(E, A, s, sp, *c4)}
    one = ShardedCeremony(be, dist, n, t, dev)
    out = []
    for kind in ("rejection_full", "proven_full", "rejection_full", "rejection_plain", "proven_plain",
                 "rejection_plain", "proven_full"):
        fresh = ShardedCeremony(be, dist, n, t, dev)
        out.append([kind, proven_summary(runs[kind](one), one), proven_summary(runs[kind](fresh), fresh)])
    return out


def main(out_path, mode=None):
    rank = int(os.environ["RANK"])
    backend = os.environ.get("DKG_DIST_BACKEND", "gloo")
    dev = torch.device("cuda", 0)
    if backend == "nccl":
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", device_id=dev)
    else:
        dist.init_process_group("gloo")
    ws = dist.get_world_size()
    be = dkg_amd.Backend(0)
    put = lambda x: torch.frombuffer(bytearray(x or b"\0"), dtype=torch.uint8).to(dev)  # noqa: E731
    out = {"mixed": mixed(be, dev, rank, ws, put)} if mode == "mixed" else scenarios(be, dev, rank, ws, put)
    dist.barrier()
    if rank == 0:
        with open(out_path, "w") as f:
            json.dump(out, f)
    be.close()
    dist.destroy_process_group()


def scenarios(be, dev, rank, ws, put):
    out = {}
    cer = faulted_ceremony(golden)
    cer["s"], cer["s_prime"] = cer.pop("shares")
    n, t = cer["n"], cer["t"]
    N = t + 1
    be.env_init(t, n)
    d0, d1 = dealer_range(rank, ws, n)
    ins = [put(cer[k][w * d0:w * d1]) for k, w in (("E", 32 * N), ("A", 32 * N), ("e1", 64 * n), ("ct", 64 * n))]
    sc = ShardedCeremony(be, dist, n, t, dev)
    for name in FULL_DIST:
        c2, c4, f3 = full_scenarios(cer)[name]
        res = sc.run_verify_full_proven(*(x.data_ptr() for x in ins), cer["sk"], cer["pk"], *lists2(c2), *lists4(c4),
                                        fetched3=None if f3 is None else f3[d0:d1])
        out["full:" + name] = proven_summary(res, sc)
    # the rejection-rule run on the same object afterwards: its block and outputs are what they were
    res = sc.run_verify_full(*(x.data_ptr() for x in ins), cer["sk"])
    out["rejection"] = dict(summary(res), exchange_bytes=sc.exchange_bytes())
    for name in PLAIN_DIST:
        pc, c4, f1, f3 = plain_scenarios(be, golden)[name]
        n, t = pc["n"], pc["t"]
        N = t + 1
        be.env_init(t, n)
        d0, d1 = dealer_range(rank, ws, n)
        pins = [put(pc[k][w * d0:w * d1]) for k, w in (("E", 32 * N), ("A", 32 * N), ("s", 32 * n), ("s_prime", 32 * n))]
        sc = ShardedCeremony(be, dist, n, t, dev)
        res = sc.run_verify_proven(*(x.data_ptr() for x in pins), *lists4(c4),
                                   fetched1=None if f1 is None else f1[d0:d1],
                                   fetched3=None if f3 is None else f3[d0:d1])
        out["plain:" + name] = proven_summary(res, sc)
    try:
        ShardedCeremony(be, dist, n, t, dev, packed=False).run_verify_proven(*(x.data_ptr() for x in pins), [], [], b"",
                                                                             b"")
        out["raw_rows"] = "accepted"
    except ValueError:
        out["raw_rows"] = "ValueError"
    return out


if __name__ == "__main__":
    main(*sys.argv[1:3])
