"""Time of the wave evaluator (receivers.hip k_pair_eval, one wave per (row, index) pair).

Sweep 1 ("c<size>"): dkg_complaints_verify and dkg_complaints3_verify with C complaints against one
dealer (and 16 x (n - 1) against sixteen) under the complaint evaluation modes 1 (per-pair Horner), 2
(difference tables), 0 (automatic) and 4 (the wave evaluator).
Sweep 2 ("pairs"): dkg_commitment_eval_pairs at (1024, 511) over the number of random pairs, its device
phases under both field multiplications, and dkg_commitment_eval at the dense shape covering the same
pairs where that is feasible.

Every call is synchronous (upload, kernels, copy back): wall-clock ms of the call, median of 5 after a
warm-up, the modes interleaved within each repetition in one process, a clock probe before and after
each step.  Each step runs in a child process under its own time limit; the tool stops at the first
step that fails.
usage: python3 tools/pairs_time.py [--out profiles/pairs_time.json] [--steps c1024,c1024t3,c256,c4096,pairs]
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
L = 2**252 + 27742317777372353535851937790883648493
SIZES = {"c1024": (1024, 511), "c1024t3": (1024, 3), "c256": (256, 127), "c4096": (4096, 2047)}
STEPS = [("c1024", 420), ("c1024t3", 300), ("c256", 240), ("c4096", 420), ("pairs", 300)]
MODES = ((1, "horner"), (2, "tables"), (0, "auto"), (4, "wave"))
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


def naf_cost(m):
    return 0 if m <= 1 else ((3 * m).bit_length() - 2) + bin((3 * m ^ m) >> 1).count("1") - 1


def chain_ops(t, x, chunk=0):
    """Dependent point operations of one wave at index x: the L - 1 steps of stage 1 (a small
    multiplication and an addition each) and, per fold stage, the multiplier's chain and the partner's
    addition."""
    import dkg_amd

    sh = dkg_amd.pair_eval_shape(t, chunk)
    ops = (sh["chunk"] - 1) * (naf_cost(x) + 1)
    if sh["stages"]:
        ops += sum(naf_cost(y) + 1 for y in dkg_amd.receiver_plan(x, t, x, sh["chunk"])["mult"])
    return ops


def complaint_step(name):
    import dkg_amd

    n, t = SIZES[name]
    N = t + 1
    be = dkg_amd.Backend(0)
    be.env_init(t, n)
    rec = {"n": n, "t": t, "device": be.pci_bus_id(), "shape": dkg_amd.pair_eval_shape(t),
           "clock_before": be.clock_probe(), "round2": {}, "round4": {}}
    master = b"\xc7" * 32
    a, b = dkg_amd.dealer_coefficients(master, 0, 0, n, t)
    big = n > 1024
    dealers = [1] if big else list(range(1, 17))
    counts = [1, n - 1] if big else sorted({min(c, n - 1) for c in (1, 16, 128, n - 1)}) + [16 * (n - 1)]
    every = [(i, q) for i in dealers for q in range(n) if q != i]
    rec["chain_ops"] = {"x%d" % x: chain_ops(t, x) for x in (1, 2, n - 1, n)}
    if big:  # the share matrices would be 2 x 512 MB: round 4 only, with arbitrary disclosed scalars (the
        # evaluation and the check do the same work whatever the verdict; the modes must still agree)
        E, A = be.share_gen(a, b, n, 1, t)[:2]
        pair = lambda i, q: (((0x9e3779b97f4a7c15 * (i * n + q + 1)) % L).to_bytes(32, "little"),) * 2  # noqa: E731
    else:
        E, A, s, sp = be.share_gen(a, b, n, n, t)
        pair = lambda i, q: (s[32 * (i * n + q):32 * (i * n + q) + 32], sp[32 * (i * n + q):32 * (i * n + q) + 32])  # noqa: E731
        sb = bytearray(s)
        for i in dealers:
            for q in range(n):
                if q != i:
                    k = 32 * (i * n + q)
                    sb[k:k + 32] = ((int.from_bytes(s[k:k + 32], "little") + 1) % L).to_bytes(32, "little")
        sk, pk = be.member_keys(master, 0, n)
        e1, ct = be.encrypt_shares(pk, bytes(sb), sp, dkg_amd.enc_randomness(master, 0, 0, n, n, t), n, n)
        Ab = bytearray(A)  # round 4: the accused dealers' A_i1 replaced, so that the held pairs accuse
        for i in dealers:
            Ab[32 * (N * i + min(1, t)):32 * (N * i + min(1, t)) + 32] = A[32 * N * 0:32 * N * 0 + 32]
        A4 = bytes(Ab)

    def enc_of(i, q):
        k = 2 * (i * n + q)
        return e1[32 * k:32 * k + 32] + ct[32 * k:32 * k + 32] + e1[32 * k + 32:32 * k + 64] + ct[32 * k + 32:32 * k + 64]

    for C in ["far"] + counts:  # "far": one complaint by receiver n (C = 1 is receiver 1, whose chains are empty)
        pairs = [(1, n - 1)] if C == "far" else every[:C]
        C, key = len(pairs), "C1far" if C == "far" else "C%d" % C
        acc, acd = [q + 1 for _, q in pairs], [i + 1 for i, _ in pairs]
        sh4 = b"".join(pair(i, q)[0] for i, q in pairs)
        rn4 = b"".join(pair(i, q)[1] for i, q in pairs)
        Ause = A if big else A4
        seen = {}

        def call4(mode):
            def run():
                be.set_complaint_eval(mode)
                out = be.complaints3_verify(n, t, acc, acd, sh4, rn4, E, Ause)
                assert seen.setdefault("r4", out) == out
            return run
        rec["round4"][key] = interleaved({label: call4(mode) for mode, label in MODES}, REPS if C < 2000 else 3)
        rec["round4"][key]["verdict0"] = seen["r4"][0].count(0)
        if big:
            continue
        enc = b"".join(enc_of(i, q) for i, q in pairs)
        w = b"".join(((0x9e3779b97f4a7c15 * (c + 1)) % L).to_bytes(32, "little") for c in range(2 * C))
        proofs = be.complaints_prove(b"".join(sk[32 * q:32 * q + 32] for _, q in pairs), enc, w)

        def call2(mode):
            def run():
                be.set_complaint_eval(mode)
                v, ql = be.complaints_verify(n, t, acc, acd, pk, E, enc, proofs)
                assert v == [0] * C and sum(ql) == n - len({i for i, _ in pairs})
            return run
        rec["round2"][key] = interleaved({label: call2(mode) for mode, label in MODES}, REPS if C < 2000 else 3)
    be.set_complaint_eval(0)
    rec["clock_after"] = be.clock_probe()
    be.close()
    return rec


def pairs_step():
    import dkg_amd

    n, t = 1024, 511
    be = dkg_amd.Backend(0)
    be.env_init(t, n)
    rec = {"n": n, "t": t, "device": be.pci_bus_id(), "shape": dkg_amd.pair_eval_shape(t),
           "clock_before": be.clock_probe(), "rows": []}
    a, b = dkg_amd.dealer_coefficients(b"\xc7" * 32, 0, 0, n, t)
    E = be.share_gen(a, b, n, 1, t)[0]
    rng = random.Random(1024)
    for count in (1, 64, 1024, 4096, 16384):
        rows = [rng.randrange(n) for _ in range(count)]
        js = [rng.randrange(n) for _ in range(count)]
        row = {"pairs": count, "distinct_rows": len(set(rows)), "distinct_indices": len(set(js))}
        ref = be.commitment_eval_pairs(n, t, rows, js, E)
        calls = {"pairs": lambda: be.commitment_eval_pairs(n, t, rows, js, E)}
        dense = sorted(set(js))
        if len(dense) <= 64:  # the dense call that covers the same pairs: M indices x all n rows
            P, _ = be.commitment_eval(n, t, dense, E)
            for p in range(count):
                e = 32 * (dense.index(js[p]) * n + rows[p])
                assert P[e:e + 32] == ref[0][32 * p:32 * p + 32]
            calls["dense"] = lambda: be.commitment_eval(n, t, dense, E)
            row["dense_indices"] = len(dense)
        row["wall_ms"] = interleaved(calls)
        be.set_streams(1)  # device phases, and the kernel under both field multiplications
        for mode, tag in ((0, "default"), (1, "prodscan"), (2, "colsum")):
            be.set_field_mode(mode)
            ph = []
            for _ in range(4):
                assert be.commitment_eval_pairs(n, t, rows, js, E) == ref
                ph.append(be.phase_times("pairs"))
            row["phase_ms_" + tag] = {k: round(statistics.median(p[k] for p in ph[1:]), 4) for k in ph[0]}
        be.set_field_mode(0)
        be.set_streams(2)
        rec["rows"].append(row)
    # one pair over chunk lengths: the chain against the work
    row = {"pairs": 1, "chunks": {}}
    be.set_streams(1)
    for chunk in (8, 16, 32, 64, 512):
        be.set_receiver_chunk(chunk)
        ph = []
        for _ in range(4):
            be.commitment_eval_pairs(n, t, [5], [682], E)
            ph.append(be.phase_times("pairs")["eval"])
        row["chunks"]["L%d" % chunk] = {"eval_ms": round(statistics.median(ph[1:]), 4), "chain_ops": chain_ops(t, 683, chunk)}
    be.set_receiver_chunk(0)
    be.set_streams(2)
    rec["rows"].append(row)
    rec["clock_after"] = be.clock_probe()
    be.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "pairs_time.json"))
    ap.add_argument("--steps", default=",".join(s for s, _ in STEPS))
    ap.add_argument("--step", help="(internal) run one step in this process and write its record to --frag")
    ap.add_argument("--frag")
    args = ap.parse_args()
    if args.step:
        rec = pairs_step() if args.step == "pairs" else complaint_step(args.step)
        with open(args.frag, "w") as f:
            json.dump(rec, f)
        return 0
    steps = args.steps.split(",")
    out = {"command": "python3 tools/pairs_time.py --steps " + ",".join(steps)}
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
    for name in SIZES:
        for rnd in ("round2", "round4"):
            for C, r in out.get(name, {}).get(rnd, {}).items():
                print(name, rnd, C, " ".join("%s %.2f" % (k, v["median"]) for k, v in r.items() if isinstance(v, dict)))
    for row in out.get("pairs", {}).get("rows", []):
        print("pairs", json.dumps(row))
    return 0


if __name__ == "__main__":
    sys.exit(main())
