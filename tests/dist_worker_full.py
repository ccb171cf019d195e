"""One rank of tests/test_gpu_dist_full.py (not a test module): full (encrypted-share) mode of the
dealer-sharded ceremony end to end through dkg_amd.distributed.ShardedCeremony.run_full /
run_verify_full on GPU 0 -- ranks sharing the GPU over gloo, or one rank over RCCL
(DKG_DIST_BACKEND=nccl), as tests/dist_worker.py.  Every FULL fixture goes through run_verify_full
(each rank uploads its dealers' commitments and ciphertexts); the two honest ones also through
run_full from their seeds.  Rank 0 writes the combined outputs as JSON to argv[1], keyed
"verify:<fixture>" / "run:<fixture>"."""
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

FULL = ["full_n4_t1.json", "full_n10_t4.json", "full_faults_n10_t4.json"]
HONEST = FULL[:2]
H = bytes.fromhex


def main(out_path):
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
    out = {}
    for name in FULL:  # received broadcasts: this rank decrypts and checks its dealers' rows
        c = golden(name)
        n, t = c["n"], c["t"]
        N = t + 1
        be.env_init(t, n)
        d0, d1 = dealer_range(rank, ws, n)
        E, A, e1, ct = (H(c[k]) for k in ("E", "A", "e1", "ct"))
        tE, tA = put(E[32 * N * d0:32 * N * d1]), put(A[32 * N * d0:32 * N * d1])
        te1, tct = put(e1[64 * n * d0:64 * n * d1]), put(ct[64 * n * d0:64 * n * d1])
        sc = ShardedCeremony(be, dist, n, t, dev)
        out["verify:" + name] = summary(sc.run_verify_full(tE.data_ptr(), tA.data_ptr(), te1.data_ptr(),
                                                           tct.data_ptr(), H(c["member_sk"])))
    for name in HONEST:  # from seeds: round 1, encryption, decryption, checks of this rank's dealers
        c = golden(name)
        n, t = c["n"], c["t"]
        be.env_init(t, n)
        d0, d1 = dealer_range(rank, ws, n)
        master = H(c["master_seed"])
        a, b = dkg_amd.dealer_coefficients(master, c["ceremony"], d0, d1 - d0, t)
        r = dkg_amd.enc_randomness(master, c["ceremony"], d0, d1 - d0, n, t)
        ta, tb, tr = put(a), put(b), put(r)  # keep all alive while the library reads them
        sc = ShardedCeremony(be, dist, n, t, dev)
        out["run:" + name] = summary(sc.run_full(ta.data_ptr(), tb.data_ptr(), tr.data_ptr(), H(c["member_sk"]),
                                                 H(c["member_pk"])))
    dist.barrier()
    if rank == 0:
        with open(out_path, "w") as f:
            json.dump(out, f)
    be.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
