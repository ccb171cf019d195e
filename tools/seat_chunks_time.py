"""Time of the seats calls under the serial walk and the chunked evaluation (receivers.hip k_seat_horner
against k_seat_chunks / k_seat_fold): dkg_verify_seats round 2, one seat per ceremony with a random
index, on the grid

  (1024, 511)  S = 1, 4, 16, 64        (256, 127)  S = 1, 16, 256
  (4096, 2047) S = 1, 2                (64, 31)    S = 1, 16, 256, 1,000

At each point: set_seat_eval mode 1, mode 2 with L forced to 8, 16, 32 and 64 (where < t + 1), mode 0, and
the loop of one verify_receivers call per seat; then the device phases "seats.decode / eval / fold / check"
(set_streams(1)) of every seats variant.  With --parent-lib (the library of a build of the parent commit)
the step "parent" times the parent's verify_seats at two grid points in the same run: the serial path has
not moved.

The commitments of a pool of at most 16 generated ceremonies (fewer at large n) are repeated to make up S
ceremonies (the work does not depend on the values); a forced chunk whose scratch would exceed 1 GiB is
listed as refused, not timed.  Every call is synchronous (upload, kernels, copy back): wall-clock
ms, median of 5 after a warm-up with min and max, all variants interleaved within each repetition in one
process, a clock probe before and after each step.  Each step runs in a child process under its own time
limit; the tool stops at the first step that fails.
usage: python3 tools/seat_chunks_time.py [--out profiles/seat_chunks_time.json] [--steps n1024,n256,n4096,n64]
                                         [--parent-lib PATH]
"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.seats_time import column, interleaved, pool_ceremonies  # noqa: E402

GRID = {"n1024": ((1024, 511), (1, 4, 16, 64)), "n256": ((256, 127), (1, 16, 256)), "n4096": ((4096, 2047), (1, 2)),
        "n64": ((64, 31), (1, 16, 256, 1000))}
STEPS = [("n1024", 400), ("n256", 300), ("n4096", 560), ("n64", 300), ("parent", 300)]
PARENT_POINTS = (("n1024", 4), ("n64", 256))
CHUNKS = (8, 16, 32, 64)
POOL = 16


def inputs(be, n, t, S, rng, pooled, pool):
    Ep, sp_, spp = pooled
    pool = min(S, pool)
    rowlen = 32 * n * (t + 1)
    E = (Ep[:rowlen * pool] * (S // pool + 1))[:rowlen * S]
    cer = list(range(S))
    js = [rng.randrange(n) for _ in range(S)]
    sc = b"".join(column(sp_, n, c % pool, j) for c, j in zip(cer, js))
    spc = b"".join(column(spp, n, c % pool, j) for c, j in zip(cer, js))
    return E, cer, js, sc, spc


def size_step(name, parent=False, only=None):
    import dkg_amd

    (n, t), seats = GRID[name]
    N = t + 1
    be = dkg_amd.Backend(0)
    be.env_init(t, n)
    rec = {"n": n, "t": t, "device": be.pci_bus_id(), "clock_before": be.clock_probe(), "points": []}
    pool = max(1, min(max(seats), POOL, (256 << 20) // (32 * n * n)))  # share matrices of at most 256 MiB
    rec["pool"] = pool
    pooled = pool_ceremonies(be, n, t, pool)
    rowlen = 32 * n * N
    for S in seats:
        if only is not None and S != only:
            continue
        rng = random.Random(n + S)  # the same indices in the parent step
        E, cer, js, sc, spc = inputs(be, n, t, S, rng, pooled, pool)
        ref = be.verify_seats(S, n, t, 2, cer, js, E, sc, spc)
        assert set(ref) <= {1, 2} and ref.count(2) == S  # honest ceremonies: ACCEPT, and SELF once per seat

        def seats_call(mode, chunk):
            def f():
                if not parent:
                    be.set_seat_eval(mode, chunk)
                assert be.verify_seats(S, n, t, 2, cer, js, E, sc, spc) == ref
            return f

        if parent:
            point = {"seats": S, "wall_ms": interleaved({"mode1": seats_call(1, 0)})}
            rec["points"].append(point)
            print(name, "parent", json.dumps(point), flush=True)
            continue
        pk = dkg_amd.seat_pack(n, js)
        point = {"n": n, "t": t, "seats": S, "waves": pk["waves"], "x_max": max(js) + 1}
        per = [(E[rowlen * c:rowlen * (c + 1)], [js[c]], sc[32 * n * c:32 * n * (c + 1)], spc[32 * n * c:32 * n * (c + 1)])
               for c in range(S)]

        def loop():
            out = b"".join(be.verify_receivers(n, t, 2, j1, Ec, s1, sp1) for Ec, j1, s1, sp1 in per)
            assert out == ref

        calls = {"mode1": seats_call(1, 0)}
        for L in CHUNKS:
            if L >= N:
                continue
            if dkg_amd.seat_eval_shape(n, t, pk["waves"], max(js) + 1, L)["scratch_bytes"] > 1 << 30:
                point.setdefault("refused_over_1GiB", []).append(L)  # the call returns DKG_E_ARG for it
                continue
            calls["mode2_L%d" % L] = seats_call(2, L)
        calls["mode0"] = seats_call(0, 0)
        calls["verify_receivers_loop"] = loop
        point["wall_ms"] = interleaved(calls)
        seats_call(0, 0)()
        point["mode0_ran"] = list(be.last_seat_eval())
        point["mode0_shape"] = {k: v for k, v in dkg_amd.seat_eval_shape(n, t, pk["waves"], max(js) + 1).items()
                                if k != "constants"}
        be.set_streams(1)  # device phases of every seats variant
        point["phase_ms"] = {}
        for label, f in calls.items():
            if label == "verify_receivers_loop":
                continue
            ph = []
            for _ in range(4):
                f()
                ph.append(be.phase_times("seats"))
            point["phase_ms"][label] = {k: round(statistics.median(p[k] for p in ph[1:]), 4)
                                        for k in ("decode", "eval", "fold", "check")}
        be.set_streams(2)
        be.set_seat_eval(0, 0)
        w = point["wall_ms"]
        forced = {k: v for k, v in w.items() if k.startswith("mode2_L")}
        best = min(forced, key=lambda k: forced[k]["median"])
        point["best_forced"] = best
        point["chunked_below_serial_disjoint"] = forced[best]["max"] < w["mode1"]["min"]
        better = min(w["mode1"], forced[best], key=lambda v: v["median"])
        point["mode0_within_spread"] = w["mode0"]["median"] <= better["max"]
        rec["points"].append(point)
        print(name, json.dumps(point), flush=True)
    rec["clock_after"] = be.clock_probe()
    be.close()
    return rec


def parent_step():
    import dkg_amd

    path = dkg_amd._lib.LIB_PATH
    rec = {"library": os.path.basename(os.path.dirname(path)) + "/" + os.path.basename(path),
           "has_seat_eval": hasattr(dkg_amd.lib(), "dkg_ctx_set_seat_eval")}
    for name, S in PARENT_POINTS:
        rec["%s_S%d" % (name, S)] = size_step(name, parent=True, only=S)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "seat_chunks_time.json"))
    ap.add_argument("--steps", default=",".join(s for s, _ in STEPS if s != "parent"))
    ap.add_argument("--parent-lib", help="libdkg_amd.so of a build of the parent commit (adds the step 'parent')")
    ap.add_argument("--step", help="(internal) run one step in this process and write its record to --frag")
    ap.add_argument("--frag")
    args = ap.parse_args()
    if args.step:
        rec = parent_step() if args.step == "parent" else size_step(args.step)
        with open(args.frag, "w") as f:
            json.dump(rec, f)
        return 0
    import dkg_amd
    steps = args.steps.split(",") + (["parent"] if args.parent_lib else [])
    out = {"command": "python3 tools/seat_chunks_time.py --steps " + ",".join(steps),
           "committed_constants": dkg_amd.seat_eval_shape(64, 31, 1, 1)["constants"], "points": []}
    with tempfile.TemporaryDirectory() as tmp:
        for name, limit in STEPS:
            if name not in steps:
                continue
            frag = os.path.join(tmp, name + ".json")
            cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--frag", frag]
            env = dict(os.environ)
            if name == "parent":
                env["DKG_AMD_LIB"] = os.path.abspath(args.parent_lib)
            try:
                rc = subprocess.run(cmd, timeout=limit, env=env).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print(f"step {name} failed (exit {rc}); stopping", file=sys.stderr)
                return 1
            with open(frag) as f:
                rec = json.load(f)
            if name == "parent":
                out["parent"] = rec
            else:
                out["points"] += rec.pop("points")
                out[name] = rec
            print(name, "done", flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
