"""Time of dkg_public_shares (pubshares.hip k_commit_colsum + the receivers' evaluator on the summed table):
the public shares of ALL n parties from the round-3 commitments, against the only route there was before.

Steps:
  "single"  B = 1, (1024, 511), js = 0..n-1;
  "batch"   B = 1,000, (64, 31), js = 0..n-1 for every ceremony.
Yardstick at the same shapes: dkg_commitment_eval(D = n, M = n) per ceremony -- the evaluation only, which is
a LOWER bound of that route, since its n^2 point additions on the host come on top.  For the batch it is
timed on 8 ceremonies and scaled by B / 8 ("yardstick_scaled_from").
Honest ceremonies (nothing reconstructed, no disclosure): pubshares.disclosed reads -1.  The batch repeats the
commitments of a pool of 256 generated ceremonies; the work does not depend on the values.

Every call is synchronous (upload, kernels, copy back): wall-clock ms, median of 5 after a warm-up, the
variants interleaved within each repetition in one process; device phases with set_streams(1), median of 3
after a warm-up; a clock probe (sclk_mhz) before and after each step.  Each step runs in a child process under
its own time limit; the tool stops at the first step that fails.
usage: python3 tools/public_shares_time.py [--out profiles/public_shares_time.json] [--steps single,batch]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"single": (1, 1024, 511), "batch": (1000, 64, 31)}
STEPS = [("single", 300), ("batch", 300)]
POOL = 256
YARD_CAP = 8  # ceremonies of the yardstick that are timed where B is larger
REPS = 5


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3),
            "count": len(xs)}


def interleaved(calls, reps=REPS):
    """calls {label: f}: one warm-up of each, then `reps` rounds that run every label once."""
    for f in calls.values():
        f()
    wall = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    return {k: spread(v) for k, v in wall.items()}


def step(name):
    import dkg_amd

    B, n, t = SHAPES[name]
    N = t + 1
    be = dkg_amd.Backend(0)
    be.env_init(t, n)
    lib = dkg_amd.lib()
    rec = {"B": B, "n": n, "t": t, "indices": n, "device": be.pci_bus_id(), "clock_before": be.clock_probe()}
    pool = min(B, POOL)
    a = b = b""
    for c in range(pool):
        ac, bc = dkg_amd.dealer_coefficients(b"\x5a" * 32, c, 0, n, t)
        a, b = a + ac, b + bc
    Ap = be.share_gen(a, b, pool * n, n, t)[1]
    del a, b
    rowlen = 32 * n * N
    A = (Ap * (B // pool + 1))[:rowlen * B]
    q = b"\x01" * (B * n)
    js = (ctypes.c_uint32 * n)(*range(n))
    V = ctypes.create_string_buffer(32 * B * n)
    st = (ctypes.c_int32 * (B * n))()
    nyard = min(B, YARD_CAP)
    P = ctypes.create_string_buffer(32 * n * n)
    ok = ctypes.create_string_buffer(n)
    rows = [A[rowlen * c:rowlen * (c + 1)] for c in range(nyard)]

    def public_shares():
        assert lib.dkg_public_shares(be.ctx, B, n, t, A, q, None, None, n, js, 0, None, None, None, None, V, st, None,
                                     None) == 0

    def yardstick():
        for r in rows:
            assert lib.dkg_commitment_eval(be.ctx, n, t, n, js, r, P, ok) == 0

    public_shares()
    assert not any(st)
    if B >= 2 * pool:  # the pool repeats
        assert V.raw[:32 * n * pool] == V.raw[32 * n * pool:64 * n * pool]
    rec["wall_ms"] = w = interleaved({"public_shares": public_shares, "commitment_eval_yardstick": yardstick})
    scale = B / nyard
    if nyard < B:
        rec["yardstick_scaled_from"] = nyard
    rec["yardstick_ms_scaled"] = round(w["commitment_eval_yardstick"]["min"] * scale, 3)
    rec["yardstick_over_public_shares"] = round(w["commitment_eval_yardstick"]["min"] * scale /
                                                w["public_shares"]["median"], 2)
    rec["below_yardstick"] = w["public_shares"]["median"] < w["commitment_eval_yardstick"]["min"] * scale
    be.set_streams(1)
    ph, phy = [], []
    for _ in range(4):
        public_shares()
        ph.append(be.phase_times("pubshares"))
        assert lib.dkg_commitment_eval(be.ctx, n, t, n, js, rows[0], P, ok) == 0
        phy.append(be.phase_times("recv"))
    rec["phase_ms"] = {k: round(statistics.median(p[k] for p in ph[1:]), 4) for k in ph[0]}
    rec["yardstick_phase_ms_one_ceremony"] = {k: round(statistics.median(p[k] for p in phy[1:]), 4)
                                              for k in ("decode", "chunks", "fold")}
    rec["receiver_chunk"] = be.last_receiver_chunk()
    be.set_streams(2)
    rec["clock_after"] = be.clock_probe()
    be.close()
    print(name, json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "public_shares_time.json"))
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
    out = {"command": "python3 tools/public_shares_time.py --steps " + ",".join(steps)}
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
            print(name, "done", flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
