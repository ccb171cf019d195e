"""Per-rank device time of the dealer-sharded ceremony under the proven-complaint rule, emulated on ONE GPU
as tools/shard_full_time.py does: rank 0 of a ws-way split owns dealers [0, n/ws) and the sharded entry
points run exactly what that rank runs.  Full (encrypted-share) mode, received broadcasts.

  a  the rejection-rule call                 dkg_ceremony_shard_verify_full_device
  b  the proven call, no complaints          dkg_ceremony_shard_verify_full_proven_device, C = C4 = 0
  c  the proven call, one owned complaint of each round per dealer (D + D), evaluation source 3: the
     complaints read the pass's own R
  d1 / d2  the same with dkg_ctx_set_complaint_eval(1) (Horner walks) / (2) (second tables) forced
  e  the only other route: the rejection-rule call, then dkg_complaints_verify and dkg_complaints3_verify on
     the owned complaints, with their host round trips (wall time; c's wall time beside it)

Device ms are the call's own (HIP events around the rank's work); five interleaved repetitions, median /
min / max; a clock probe before and after.  One GPU: nothing here has run on distinct devices.
usage: python3 tools/shard_proven_time.py [n t] [--ws 8] [--reps 5] [--out profiles/shard_proven_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MASTER = b"\xbd" * 32


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3),
            "count": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int, nargs="?", default=1024)
    ap.add_argument("t", type=int, nargs="?", default=511)
    ap.add_argument("--ws", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "shard_proven_time.json"))
    args = ap.parse_args()
    import torch

    import dkg_amd

    n, t, ws, reps = args.n, args.t, args.ws, args.reps
    N, D = t + 1, n // ws
    be = dkg_amd.Backend(0)
    rec = {"n": n, "t": t, "ws": ws, "dealers": D, "device": be.pci_bus_id(), "reps": reps,
           "clock_before": be.clock_probe()}
    be.env_init(t, n)
    u8 = dict(dtype=torch.uint8, device=torch.device("cuda", 0))
    ta, tb = torch.empty(32 * D * N, **u8), torch.empty(32 * D * N, **u8)
    tr = torch.empty(64 * D * n, **u8)
    be.dealer_coefficients_device(MASTER, 0, 1, 0, D, t, ta.data_ptr(), tb.data_ptr())
    be.enc_randomness_device(MASTER, 0, 1, 0, D, n, t, tr.data_ptr())
    tE, tA = torch.empty(32 * D * N, **u8), torch.empty(32 * D * N, **u8)
    ts, tsp = torch.empty(32 * D * n, **u8), torch.empty(32 * D * n, **u8)
    be.share_gen_device(D, n, t, ta.data_ptr(), tb.data_ptr(), tE.data_ptr(), tA.data_ptr(), ts.data_ptr(),
                        tsp.data_ptr())
    host = lambda x: bytes(x.cpu().numpy())  # noqa: E731
    s, sp, E, A = host(ts), host(tsp), host(tE), host(tA)
    sk, pk = be.member_keys(MASTER, 0, n)
    e1, ct = be.encrypt_shares(pk, s, sp, host(tr), D, n)
    te1, tct = (torch.frombuffer(bytearray(x), dtype=torch.uint8).to("cuda:0") for x in (e1, ct))
    # one complaint of each round per dealer, by a receiver that is not the dealer: honest pairs, so every
    # verdict is FalseClaimedInequality (2) -- the full verification runs
    pairs = [((37 * i + 5) % n + 1, i + 1) for i in range(D)]
    assert all(j != i for j, i in pairs)

    def enc_of(i, q):
        k = 2 * (i * n + q)
        return e1[32 * k:32 * k + 32] + ct[32 * k:32 * k + 32] + e1[32 * k + 32:32 * k + 64] + ct[32 * k + 32:32 * k + 64]

    enc = b"".join(enc_of(i - 1, j - 1) for j, i in pairs)
    proofs = be.complaints_prove(b"".join(sk[32 * (j - 1):32 * j] for j, _ in pairs), enc, bytes([9]) * (64 * D))
    acc, acd = [j for j, _ in pairs], [i for _, i in pairs]
    sh4 = b"".join(s[32 * ((i - 1) * n + j - 1):32 * ((i - 1) * n + j)] for j, i in pairs)
    rn4 = b"".join(sp[32 * ((i - 1) * n + j - 1):32 * ((i - 1) * n + j)] for j, i in pairs)
    o2, o4 = torch.empty(D * n, **u8), torch.empty(D * n, **u8)
    oA, op = torch.empty(D * 32, **u8), torch.empty(n * 32, **u8)
    fl = torch.empty(D, dtype=torch.int32, device="cuda:0")
    ds = torch.empty(n, dtype=torch.int32, device="cuda:0")
    ins = (tE.data_ptr(), tA.data_ptr(), te1.data_ptr(), tct.data_ptr())
    outs = (o2.data_ptr(), o4.data_ptr(), oA.data_ptr(), op.data_ptr())
    # the single-ceremony primitives of route e take the ceremony's [n] commitment rows: the rank's rows first
    En, An = E + bytes(32 * N * (n - D)), A + bytes(32 * N * (n - D))

    def rejection():
        w0 = time.perf_counter()
        ms = be.ceremony_shard_verify_full_device(n, t, 0, D, *ins, sk, *outs)
        return ms, (time.perf_counter() - w0) * 1e3

    def proven(with_complaints):
        c2 = (acc, acd, proofs) if with_complaints else ([], [], b"")
        c4 = (acc, acd, sh4, rn4) if with_complaints else ([], [], b"", b"")
        w0 = time.perf_counter()
        ms, v, v4 = be.ceremony_shard_verify_full_proven_device(n, t, 0, D, *ins, sk, pk, *c2, *c4, *outs, D,
                                                                fl.data_ptr(), ds.data_ptr())
        return ms, (time.perf_counter() - w0) * 1e3, v, v4, be.last_complaint_eval()

    def route_e():
        w0 = time.perf_counter()
        ms = be.ceremony_shard_verify_full_device(n, t, 0, D, *ins, sk, *outs)
        v, _ = be.complaints_verify(n, t, acc, acd, pk, En, enc, proofs)
        v4, _ = be.complaints3_verify(n, t, acc, acd, sh4, rn4, En, An)
        return ms, (time.perf_counter() - w0) * 1e3, v, v4

    be.set_complaint_eval(0)
    rejection(), proven(False), route_e()  # warm every path's buffers
    ref = proven(True)
    assert ref[2] == [2] * D and ref[3] == [2] * D and ref[4] == 3, ref[2:]
    for mode in (1, 2):
        be.set_complaint_eval(mode)
        got = proven(True)
        assert got[2:4] == ref[2:4] and got[4] == mode, (mode, got[4])
    be.set_complaint_eval(0)
    assert route_e()[2:] == ref[2:4]
    dev = {k: [] for k in ("a_rejection", "b_proven_no_complaints", "c_proven_source3", "d1_proven_horner",
                           "d2_proven_tables")}
    wall = {k: [] for k in ("c_proven_source3", "e_rejection_then_primitives")}
    for _ in range(reps):  # interleaved, so that drift hits every configuration alike
        dev["a_rejection"].append(rejection()[0])
        dev["b_proven_no_complaints"].append(proven(False)[0])
        r = proven(True)
        dev["c_proven_source3"].append(r[0])
        wall["c_proven_source3"].append(r[1])
        for mode, key in ((1, "d1_proven_horner"), (2, "d2_proven_tables")):
            be.set_complaint_eval(mode)
            dev[key].append(proven(True)[0])
        be.set_complaint_eval(0)
        wall["e_rejection_then_primitives"].append(route_e()[1])
    rec["complaints_owned"] = {"round2": D, "round4": D}
    rec["device_ms"] = {k: spread(v) for k, v in dev.items()}
    rec["wall_ms"] = {k: spread(v) for k, v in wall.items()}
    rec["last_split"] = be.last_split()
    rec["clock_after"] = be.clock_probe()
    rec["note"] = ("one GPU emulating rank 0 of %d; nothing here has run on distinct devices.  Route e's wall time "
                   "includes the primitives' uploads of the ceremony's [n] commitment rows." % ws)
    be.close()
    print(json.dumps({k: rec[k] for k in ("device_ms", "wall_ms")}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
