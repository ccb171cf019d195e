"""Device time of a batch of full-mode (encrypted-share) ceremonies, against the only other route to
the same work -- one dkg_ceremony_run_full_device call per ceremony with that ceremony's keys -- and
the batched decryption chain against the single n = 1024 ceremony's (the same width-4 chain).

Coefficients, encryption randomness and keys are seeded on the device before anything is timed.
usage: python3 tools/batch_full_time.py --B 10000 --n 64 --t 31 [--steps K] [--loop 200] [--chunk C]
                                        [--out profiles/batch_full_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4),
            "count": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=10000)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--t", type=int, default=31)
    ap.add_argument("--steps", type=int, default=0, help="timed batches (0: at least 3, until the window reaches 1 s)")
    ap.add_argument("--loop", type=int, default=200, help="ceremonies of the one-call-per-ceremony loop")
    ap.add_argument("--chunk", type=int, default=0, help="dkg_ctx_set_batch_full_chunk (0: automatic)")
    ap.add_argument("--single-n", type=int, default=1024, help="single ceremony whose full.dec_mul is the yardstick (0: skip)")
    ap.add_argument("--out", default=os.path.join("profiles", "batch_full_time.json"))
    args = ap.parse_args()
    import torch

    import dkg_amd
    from dkg_amd import _lib

    B, n, t = args.B, args.n, args.t
    N = t + 1
    master = b"\xbf" * 32
    dev = torch.device("cuda", 0)
    be = dkg_amd.Backend(0)
    be.env_init(t, n)
    be.set_batch_full_chunk(args.chunk)
    ta = torch.empty(32 * B * n * N, dtype=torch.uint8, device=dev)
    tb = torch.empty_like(ta)
    tr = torch.empty(64 * B * n * n, dtype=torch.uint8, device=dev)
    be.dealer_coefficients_device(master, 0, B, 0, n, t, ta.data_ptr(), tb.data_ptr())
    be.enc_randomness_device(master, 0, B, 0, n, n, t, tr.data_ptr())
    t0 = time.perf_counter()
    sk, pk = be.member_keys_batch(master, 0, B, n)
    keys_s = time.perf_counter() - t0
    rec = {"B": B, "n": n, "t": t, "chunk": args.chunk, "device": be.pci_bus_id(), "member_keys_batch_s": round(keys_s, 3),
           "clock_before": be.clock_probe()}

    def batch():
        w0 = time.perf_counter()
        r = dkg_amd.ceremony_batch_full_device(be, B, n, t, ta.data_ptr(), tb.data_ptr(), tr.data_ptr(), sk, pk)
        wall = (time.perf_counter() - w0) * 1e3
        assert r.n_qualified == [n] * B, "an honest full-mode ceremony lost a dealer"
        return r, wall

    batch()  # warm-up: allocations, code objects
    ms, walls, phases = [], [], []
    while len(ms) < (args.steps or 3) or (not args.steps and sum(ms) < 1000.0):
        r, wall = batch()
        ms.append(r.ms["total"])
        walls.append(wall)
        phases.append(dict(be.batch_full_phase_times(), round1=r.ms["round1"], checks=r.ms["checks"],
                           round3=r.ms["round3"], finalise=r.ms["finalise"]))
    items = 2 * B * n * n
    med = {k: statistics.median(p[k] for p in phases) for k in phases[0]}
    rec["batch"] = {"device_ms": spread(ms), "wall_ms": spread(walls), "window_ms": round(sum(ms), 1),
                    "per_ceremony_ms": round(statistics.median(ms) / B, 5), "items": items,
                    "phase_ms_median": {k: round(v, 3) for k, v in med.items()},
                    "per_item_ns": {k: round(v * 1e6 / items, 3) for k, v in med.items() if k.startswith(("enc_", "dec_"))},
                    "per_item_ns_spread": {k: spread([p[k] * 1e6 / items for p in phases]) for k in ("enc_mul", "dec_mul")}}
    rec["clock_after_batch"] = be.clock_probe()

    # the loop a caller without the batch API runs: one call per ceremony, each with its own keys
    loop = min(args.loop, B)
    lw, ld = [], []
    for rep in range(2):  # the first pass warms the single path's buffers
        lw, ld = [], []
        for c in range(loop):
            a = ta[32 * n * N * c:32 * n * N * (c + 1)]
            b = tb[32 * n * N * c:32 * n * N * (c + 1)]
            rr = tr[64 * n * n * c:64 * n * n * (c + 1)]
            w0 = time.perf_counter()
            one = be.ceremony_full_device(a.data_ptr(), b.data_ptr(), rr.data_ptr(), sk[32 * n * c:32 * n * (c + 1)],
                                          pk[32 * n * c:32 * n * (c + 1)], n, t)
            lw.append((time.perf_counter() - w0) * 1e3)
            ld.append(one.ms["total"])
            assert one.n_qualified == n
    rec["single_loop"] = {"ceremonies": loop, "device_ms_per_ceremony": spread(ld), "wall_ms_per_ceremony": spread(lw)}
    rec["batch_vs_loop"] = {"device": round(statistics.median(ld) / (statistics.median(ms) / B), 2),
                            "loop_wall_over_batch_wall": round(statistics.median(lw) / (statistics.median(walls) / B), 2)}

    if args.single_n:  # the same decryption chain in the single ceremony, serialised so that its phases are timed
        sn, st = args.single_n, (args.single_n - 1) // 2
        be.env_init(st, sn)
        be.set_streams(1)
        sa = torch.empty(32 * sn * (st + 1), dtype=torch.uint8, device=dev)
        sb = torch.empty_like(sa)
        sr = torch.empty(64 * sn * sn, dtype=torch.uint8, device=dev)
        be.dealer_coefficients_device(master, 0, 1, 0, sn, st, sa.data_ptr(), sb.data_ptr())
        be.enc_randomness_device(master, 0, 1, 0, sn, sn, st, sr.data_ptr())
        ssk, spk = be.member_keys(master, 0, sn)
        dm = []
        for _ in range(4):
            be.ceremony_full_device(sa.data_ptr(), sb.data_ptr(), sr.data_ptr(), ssk, spk, sn, st)
            dm.append(_lib.lib().dkg_ctx_phase_ms(be.ctx, b"full.dec_mul"))
        dm = dm[1:]  # the first call allocates
        sitems = 2 * sn * sn
        rec["single_dec_mul"] = {"n": sn, "t": st, "items": sitems, "ms": spread(dm),
                                 "per_item_ns": spread([v * 1e6 / sitems for v in dm])}
        y = statistics.median(dm) * 1e6 / sitems
        rec["dec_mul_batched_over_single"] = round(rec["batch"]["per_item_ns"]["dec_mul"] / y, 3)
        rec["clock_after_single"] = be.clock_probe()
    rec["enc_mul_over_dec_mul"] = round(rec["batch"]["per_item_ns"]["enc_mul"] / rec["batch"]["per_item_ns"]["dec_mul"], 3)
    be.close()
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
