"""Time of party_round1_seats (seat_deal.hip k_seat_enc_mul): an operator's seats deal round 1 in one
call, one seat per ceremony with a random index, under both routes of K = pk r, against what the operator
could do before -- one share_gen(D = 1) + one encrypt_shares(D = 1) per seat.

Steps: "s1000" 1,000 seats of (64, 31); "s10000" 10,000 seats of (64, 31); "n1024" 16 seats of (1024, 511).
Per step, in one process:
  modes 1 (a radix-16 comb per key slot) and 2 (the joint chain) interleaved over ROUNDS rounds after one
  warm-up of each, the order of the two swapped from round to round: whole-call wall-clock ms (upload, kernels, copy back) and the device phases
  (set_streams(1): seats.commit, deal_e1, deal_mul, deal_encode, deal_sym) with their sum per call
  ("device_ms": the call without its host copies), each as median / min / max;
  the per-seat loop on the first `loop_seats` seats, timed in the same rounds and scaled by S / loop_seats
  ("loop_scaled_from"); a clock probe before and after.
The member keys of a pool of at most 256 ceremonies are repeated to make up S ceremonies (the work does
not depend on the values; every ceremony's keys are still uploaded and decoded).  Outputs of the two
routes are compared once, and the loop's rows with the call's.
Each step runs in a child process under its own time limit; the tool stops at the first step that fails.
usage: python3 tools/seat_deal_time.py [--out profiles/seat_deal_time.json] [--steps s1000,s10000,n1024]
"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"s1000": (1000, 64, 31, 32), "s10000": (10000, 64, 31, 32), "n1024": (16, 1024, 511, 4)}  # S, n, t, loop
STEPS = [("s1000", 300), ("s10000", 420), ("n1024", 420)]
POOL = 256
ROUNDS = 10
PHASES = ("commit", "deal_e1", "deal_mul", "deal_encode", "deal_sym")


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3),
            "count": len(xs)}


def scalars(rng, count):
    """count canonical scalars (below 2^252), 32 bytes each."""
    raw = bytearray(rng.randbytes(32 * count))
    raw[31::32] = bytes(b & 0x0F for b in raw[31::32])
    return bytes(raw)


def step(name):
    import dkg_amd

    S, n, t, nloop = SHAPES[name]
    N = t + 1
    be = dkg_amd.Backend(0)
    be.env_init(t, n)
    be.set_streams(1)  # the call runs on one stream either way; this records its phases
    rng = random.Random(S + n)
    pool = min(S, POOL)
    _, pkp = be.member_keys_batch(b"\xd1" * 32, 0, pool, n)
    pk = (pkp * (S // pool + 1))[:32 * n * S]
    cer = list(range(S))
    js = [rng.randrange(n) for _ in range(S)]
    a, b, r = scalars(rng, S * N), scalars(rng, S * N), scalars(rng, 2 * S * n)
    rec = {"seats": S, "n": n, "t": t, "keys": S * n, "device": be.pci_bus_id(), "pool": pool, "rounds": ROUNDS,
           "loop_seats": nloop, "loop_scaled_from": nloop, "clock_before": be.clock_probe()}

    def call(mode):
        be.set_seat_deal(mode)
        out = be.party_round1_seats(S, n, t, cer, js, a, b, r, pk)
        assert be.last_seat_deal() == mode
        return out

    def loop():
        rows = []
        for p in range(nloop):
            E, A, s, sp = be.share_gen(a[32 * N * p:32 * N * (p + 1)], b[32 * N * p:32 * N * (p + 1)], 1, n, t)
            e1, ct = be.encrypt_shares(pk[32 * n * p:32 * n * (p + 1)], s, sp, r[64 * n * p:64 * n * (p + 1)], 1, n)
            rows.append((E, e1, ct))
        return rows

    ref = {m: call(m) for m in (1, 2)}  # the warm-up of each, compared
    assert all(ref[1][k] == ref[2][k] for k in ref[1]), "the routes differ"
    rows = loop()
    for p, (E, e1, ct) in enumerate(rows):
        assert ref[2]["E"][32 * N * p:32 * N * (p + 1)] == E
        assert ref[2]["e1"][64 * n * p:64 * n * (p + 1)] == e1 and ref[2]["ct"][64 * n * p:64 * n * (p + 1)] == ct
    del ref, rows
    wall = {1: [], 2: [], "loop": []}
    phases = {1: {k: [] for k in PHASES}, 2: {k: [] for k in PHASES}}
    for rnd in range(ROUNDS):
        for m in ((1, 2) if rnd % 2 == 0 else (2, 1)):  # a mode is first in every other round
            t0 = time.perf_counter()
            call(m)
            wall[m].append((time.perf_counter() - t0) * 1e3)
            ph = be.phase_times("seats")
            for k in PHASES:
                phases[m][k].append(ph[k])
        t0 = time.perf_counter()
        loop()
        wall["loop"].append((time.perf_counter() - t0) * 1e3)
    be.set_seat_deal(0)
    for m in (1, 2):
        device = [sum(phases[m][k][i] for k in PHASES) for i in range(ROUNDS)]  # the call's kernels, per round
        rec[f"mode{m}"] = {"call_ms": spread(wall[m]), "call_ms_by_round": [round(v, 2) for v in wall[m]],
                           "device_ms": spread(device),
                           "phase_ms": {k: spread(v) for k, v in phases[m].items()}}
    rec["per_seat_loop"] = {"sample_ms": spread(wall["loop"]),
                            "scaled_ms": spread([v * S / nloop for v in wall["loop"]])}
    rec["mode2_median_below_mode1_min"] = {
        k: rec["mode2"][k]["median"] < rec["mode1"][k]["min"] for k in ("call_ms", "device_ms")}
    rec["mode2_median_below_mode1_min"]["deal_mul"] = (
        rec["mode2"]["phase_ms"]["deal_mul"]["median"] < rec["mode1"]["phase_ms"]["deal_mul"]["min"])
    rec["clock_after"] = be.clock_probe()
    be.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "seat_deal_time.json"))
    ap.add_argument("--steps", default=",".join(s for s, _ in STEPS))
    ap.add_argument("--step", help="(internal) run one step in this process and write its record to --frag")
    ap.add_argument("--frag")
    args = ap.parse_args()
    if args.step:
        rec = step(args.step)
        with open(args.frag, "w") as f:
            json.dump(rec, f)
        return 0
    steps = args.steps.split(",")
    out = {"command": "python3 tools/seat_deal_time.py --steps " + ",".join(steps)}
    if os.path.exists(args.out):  # steps run in several visits accumulate in one record
        with open(args.out) as f:
            out.update({k: v for k, v in json.load(f).items() if k != "command"})
    with tempfile.TemporaryDirectory() as tmp:
        for name, limit in STEPS:
            if name not in steps:
                continue
            frag = os.path.join(tmp, name + ".json")
            cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--frag", frag]
            try:
                rc = subprocess.run(cmd, timeout=limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print(f"step {name} failed (exit {rc}); stopping", file=sys.stderr)
                return 1
            with open(frag) as f:
                out[name] = json.load(f)
            print(name, json.dumps(out[name]), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
