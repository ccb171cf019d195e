"""Time of one party's share checks: dkg_verify_receiver (the serial walk, one dependent chain per
dealer) against dkg_verify_receivers (chunked evaluation, receivers.hip) with one index, over chunk
lengths; several indices in one call against as many calls; dkg_party_round2.  The sweep is what the
constants of dkg_receiver_plan_for's rule are fitted to (the record's "fit").

Every call is synchronous (upload, kernels, copy back): wall-clock ms of the call and the device ms of
its recv.* phases (one stream), medians after a warm-up, with a clock probe before and after.  Each
step runs in a child process under its own time limit; the tool stops at the first step that fails.
usage: python3 tools/receivers_time.py [--out profiles/receivers_time.json] [--steps s64,s256,...]
                                       [--parent-tree DIR]   (a built checkout of the parent commit: step "parent")
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# step "parent": the package and library of a checkout of the parent commit, built in place
sys.path.insert(0, os.environ.get("DKG_RECV_PARENT_TREE") or ROOT)
L = 2**252 + 27742317777372353535851937790883648493
SIZES = {"s64": (64, 31), "s256": (256, 127), "s1024": (1024, 511), "s1024t3": (1024, 3), "s4096": (4096, 2047)}
STEPS = [("s64", 200), ("s256", 200), ("s1024", 300), ("s1024t3", 200), ("s4096", 560), ("multi", 300), ("party", 300),
         ("parent", 300)]
CHUNKS = (2, 4, 8, 16, 32, 64)  # 2 only where t + 1 <= 8
REPS = 5


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3),
            "count": len(xs)}


def timed(f, reps=REPS, phases=None, be=None):
    """Wall ms of f with the context's default streams; with `phases`, the device phases of three more
    calls on one stream (the only mode that records them)."""
    f()  # warm-up: allocations, code objects
    wall, ph = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        wall.append((time.perf_counter() - t0) * 1e3)
    out = {"wall_ms": spread(wall)}
    if phases:
        be.set_streams(1)
        for _ in range(3):
            f()
            ph.append(phases())
        be.set_streams(2)
        out["phase_ms"] = {k: round(statistics.median(p[k] for p in ph), 4) for k in ph[0]}
    return out


def indices(n):
    """x = n (one NAF digit), n - 1, and a dense-NAF index (10101..b)."""
    return [n, n - 1, int("10" * 16, 2) >> (32 - n.bit_length() + 1) | 1 if n > 4 else 1]


def naf_cost(m):
    return 0 if m <= 1 else ((3 * m).bit_length() - 2) + bin((3 * m ^ m) >> 1).count("1") - 1


def features(n, t, x, plan):
    """(launches, dependent point operations, lane operations) of the evaluation under `plan`."""
    N, lanes = t + 1, (n + 63) // 64 * 64
    Lc = min(plan["chunk"], N)
    G = -(-N // Lc)
    cx = naf_cost(x) + 1
    launches, chain, work = 1, (Lc - 1) * cx, lanes * (N - G) * cx
    for r, y in zip(plan["arity"], plan["mult"]):
        Gout = -(-G // r)
        cy = naf_cost(y) + 1
        launches, chain, work = launches + 1, chain + (r - 1) * cy, work + lanes * (G - Gout) * cy
        G = Gout
    return launches, chain, work


def committee(be, n, t):
    """Seeded commitments and the share columns of the indices in indices(n): E, A, {x: (s, sp)}."""
    import dkg_amd

    master = b"\xa3" * 32
    a, b = dkg_amd.dealer_coefficients(master, 0, 0, n, t)
    cols = {}
    if n <= 1024:
        E, A, s, sp = be.share_gen(a, b, n, n, t)
        for x in set(indices(n)):
            j = x - 1
            cols[x] = tuple(b"".join(m[32 * (i * n + j):32 * (i * n + j) + 32] for i in range(n)) for m in (s, sp))
    else:  # the share matrices would be 2 x 512 MB: arbitrary canonical shares (every pair rejected; the
        # work of the check does not depend on its outcome, and both calls must still agree)
        E, A = be.share_gen(a, b, n, 1, t)[:2]
        for x in set(indices(n)):
            col = b"".join(((0x9e3779b97f4a7c15 * (i + x)) % L).to_bytes(32, "little") for i in range(n))
            cols[x] = (col, col)
    return E, A, cols


def recv_phases(be):
    return lambda: be.phase_times("recv")


def size_step(name, field_ab):
    import dkg_amd

    n, t = SIZES[name]
    be = dkg_amd.Backend(0)
    be.env_init(t, n)
    rec = {"n": n, "t": t, "device": be.pci_bus_id(), "clock_before": be.clock_probe(), "rows": []}
    E, A, cols = committee(be, n, t)
    for rnd, C in ((2, E), (4, A)):
        for x in indices(n):
            s, sp = cols[x]
            spa = sp if rnd == 2 else None
            ref = be.verify_receiver(n, t, rnd, x - 1, C, s, spa)
            row = {"round": rnd, "x": x,
                   "verify_receiver": timed(lambda: be.verify_receiver(n, t, rnd, x - 1, C, s, spa))}
            for label, chunk in [("auto", 0), ("serial", t + 1)] + [("L%d" % c, c) for c in CHUNKS if c < t + 1 and (c > 2 or t < 8)]:
                be.set_receiver_chunk(chunk)
                assert be.verify_receivers(n, t, rnd, [x - 1], C, s, spa) == ref
                r = timed(lambda: be.verify_receivers(n, t, rnd, [x - 1], C, s, spa), phases=recv_phases(be), be=be)
                plan = dkg_amd.receiver_plan(n, t, x, chunk)
                r["chunk"], r["stages"] = be.last_receiver_chunk(), plan["stages"]
                r["launches"], r["chain_ops"], r["lane_ops"] = features(n, t, x, plan)
                row[label] = r
            if field_ab and rnd == 2:
                for mode, tag in ((1, "prodscan"), (2, "colsum")):
                    be.set_field_mode(mode)
                    for label, chunk in (("auto", 0), ("L8", 8)):
                        if chunk >= t + 1:
                            continue
                        be.set_receiver_chunk(chunk)
                        row["%s_%s" % (label, tag)] = timed(lambda: be.verify_receivers(n, t, rnd, [x - 1], C, s, spa),
                                                            phases=recv_phases(be), be=be)
                be.set_field_mode(0)
            be.set_receiver_chunk(0)
            rec["rows"].append(row)
    rec["clock_after"] = be.clock_probe()
    be.close()
    return rec


def multi_step():
    import dkg_amd

    n, t = 1024, 511
    be = dkg_amd.Backend(0)
    be.env_init(t, n)
    rec = {"n": n, "t": t, "device": be.pci_bus_id(), "clock_before": be.clock_probe()}
    a, b = dkg_amd.dealer_coefficients(b"\xa3" * 32, 0, 0, n, t)
    E, A, s, sp = be.share_gen(a, b, n, n, t)
    col = lambda m, j: b"".join(m[32 * (i * n + j):32 * (i * n + j) + 32] for i in range(n))  # noqa: E731
    for M in (8, 64):
        js = [(j * 997 + 5) % n for j in range(M)]
        sc, spc = b"".join(col(s, j) for j in js), b"".join(col(sp, j) for j in js)

        def separate():
            return b"".join(be.verify_receiver(n, t, 2, j, E, sc[32 * n * m:32 * n * (m + 1)],
                                               spc[32 * n * m:32 * n * (m + 1)]) for m, j in enumerate(js))

        def separate_new():
            return b"".join(be.verify_receivers(n, t, 2, [j], E, sc[32 * n * m:32 * n * (m + 1)],
                                                spc[32 * n * m:32 * n * (m + 1)]) for m, j in enumerate(js))
        assert be.verify_receivers(n, t, 2, js, E, sc, spc) == separate()
        rec["M%d" % M] = {"one_call": timed(lambda: be.verify_receivers(n, t, 2, js, E, sc, spc), 5, recv_phases(be), be),
                          "calls_verify_receivers": timed(separate_new, 3),
                          "calls_verify_receiver": timed(separate, 3 if M == 8 else 1)}
    rec["clock_after"] = be.clock_probe()
    be.close()
    return rec


def party_step():
    import dkg_amd

    n, t, j = 1024, 511, 340
    be = dkg_amd.Backend(0)
    be.env_init(t, n)
    rec = {"n": n, "t": t, "device": be.pci_bus_id(), "clock_before": be.clock_probe()}
    master = b"\xa3" * 32
    a, b = dkg_amd.dealer_coefficients(master, 0, 0, n, t)
    E, A, s, sp = be.share_gen(a, b, n, n, t)
    sk, pk = be.member_keys(master, 0, n)
    r = dkg_amd.enc_randomness(master, 0, 0, n, n, t)
    w = b"".join(((0x9e3779b97f4a7c15 * (c + 1)) % L).to_bytes(32, "little") for c in range(2 * n))
    for cheats in (0, 16):
        sb = bytearray(s)
        for i in range(cheats):
            k = 32 * ((i * 61 + 2) * n + j)
            sb[k:k + 32] = ((int.from_bytes(sb[k:k + 32], "little") + 1) % L).to_bytes(32, "little")
        e1, ct = be.encrypt_shares(pk, bytes(sb), sp, r, n, n)
        e1c = b"".join(e1[64 * (i * n + j):64 * (i * n + j) + 64] for i in range(n))
        ctc = b"".join(ct[64 * (i * n + j):64 * (i * n + j) + 64] for i in range(n))
        out = be.party_round2(n, t, j, E, e1c, ctc, sk[32 * j:32 * j + 32], w)
        assert out["complaints"] == cheats and not out["r2_error"]
        rec["rejected_%d" % cheats] = timed(lambda: be.party_round2(n, t, j, E, e1c, ctc, sk[32 * j:32 * j + 32], w),
                                            5, recv_phases(be), be)
    rec["clock_after"] = be.clock_probe()
    be.close()
    return rec


def parent_step():
    """dkg_verify_receiver alone, through the package of --parent-tree (the parent commit's build)."""
    import dkg_amd

    rec = {"package": os.path.relpath(os.path.dirname(dkg_amd.__file__), ROOT)}
    for name in ("s1024", "s256"):
        n, t = SIZES[name]
        be = dkg_amd.Backend(0)
        be.env_init(t, n)
        E, A, cols = committee(be, n, t)
        rec[name] = {"clock_before": be.clock_probe()}
        for x in indices(n):
            s, sp = cols[x]
            rec[name]["x%d" % x] = timed(lambda: be.verify_receiver(n, t, 2, x - 1, E, s, sp))
        rec[name]["clock_after"] = be.clock_probe()
        be.close()
    return rec


def fit(out):
    """Least squares of the evaluation's device time (recv.chunks + recv.fold, us) over every forced
    configuration of the sweep: launches, dependent operations, lane operations."""
    import numpy as np

    X, y, ser, setup = [], [], [], []
    ev = lambda r: 1e3 * (r["phase_ms"]["chunks"] + max(r["phase_ms"]["fold"], 0.0))  # noqa: E731
    for name in SIZES:
        for row in out.get(name, {}).get("rows", []):
            for label, r in row.items():  # what a plan with stages costs the call beyond its kernels
                if isinstance(r, dict) and r.get("stages") and label != "auto":
                    setup.append(1e3 * (r["wall_ms"]["median"] - row["serial"]["wall_ms"]["median"]) -
                                 (ev(r) - ev(row["serial"])))
            for label, r in row.items():
                if isinstance(r, dict) and "launches" in r and label != "auto":
                    p = r["phase_ms"]
                    us = 1e3 * (p["chunks"] + max(p["fold"], 0.0))
                    if r["stages"] == 0:  # k_horner: a kernel of its own, priced by its own latency
                        ser.append((r["launches"], r["chain_ops"], r["lane_ops"], us))
                        continue
                    X.append([r["launches"], r["chain_ops"], r["lane_ops"]])
                    y.append(us)
    if len(X) < 6:
        return None
    X, y = np.array(X, float), np.array(y, float)
    # relative error: the small configurations matter as much as the large ones
    c, *_ = np.linalg.lstsq(X / y[:, None], np.ones(len(y)), rcond=None)
    pred = X @ c
    slat = [(us - c[0] * la - c[2] * w) / ch for la, ch, w, us in ser if ch]
    return {"chunked_setup_us": round(float(np.median(setup)), 2) if setup else None,
            "serial_op_latency_us": round(float(np.median(slat)), 4) if slat else None,"launch_us": round(float(c[0]), 3), "op_latency_us": round(float(c[1]), 4), "lane_op_us": float("%.4g" % c[2]),
            "points": len(y), "median_rel_err": round(float(np.median(np.abs(pred - y) / y)), 3),
            "max_rel_err": round(float(np.max(np.abs(pred - y) / y)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "receivers_time.json"))
    ap.add_argument("--steps", default=",".join(s for s, _ in STEPS if s != "parent"))
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit (adds the step 'parent')")
    ap.add_argument("--step", help="(internal) run one step in this process and write its record to --frag")
    ap.add_argument("--frag")
    args = ap.parse_args()
    if args.step:
        if args.step in SIZES:
            rec = size_step(args.step, args.step in ("s1024", "s4096"))
        else:
            rec = {"multi": multi_step, "party": party_step, "parent": parent_step}[args.step]()
        with open(args.frag, "w") as f:
            json.dump(rec, f)
        return 0
    import dkg_amd
    steps = args.steps.split(",") + (["parent"] if args.parent_tree else [])
    out = {"command": "python3 tools/receivers_time.py --steps " + ",".join(steps),
           "committed_constants": dkg_amd.receiver_plan_constants()}
    with tempfile.TemporaryDirectory() as tmp:
        for name, limit in STEPS:
            if name not in steps:
                continue
            frag = os.path.join(tmp, name + ".json")
            cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--frag", frag]
            env = dict(os.environ)
            if name == "parent":
                env["DKG_RECV_PARENT_TREE"] = os.path.abspath(args.parent_tree)
            try:
                rc = subprocess.run(cmd, timeout=limit, env=env).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print(f"step {name} failed (exit {rc}); stopping", file=sys.stderr)
                return 1
            with open(frag) as f:
                out[name] = json.load(f)
            print(name, "done", flush=True)
    out["fit"] = fit(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    # the table a reader wants first
    for name in SIZES:
        for row in out.get(name, {}).get("rows", []):
            cells = ["%s %.2f" % (k, v["wall_ms"]["median"]) for k, v in row.items() if isinstance(v, dict)]
            print(name, "r%d x=%d |" % (row["round"], row["x"]), " ".join(cells))
    print("fit", json.dumps(out["fit"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
