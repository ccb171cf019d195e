"""Time of the batched round-4 complaint verification (dkg_complaints3_verify) at n = 1024, against the
host-driven primitive it stands beside (dkg_complaint3_verify) on the same inputs in the same process,
and the A/B of its evaluations of P^E_i(j), P^A_i(j): per-pair Horner (mode 1), the difference tables of
the accused dealer's two rows (mode 2), and what the automatic mode (0) picks with the constants fitted
for round 1 (runtime.hip complaint_tables_pay).

Every call here is synchronous (uploads, kernels, the copy back), so the figures are wall-clock
milliseconds of the call, medians after a warm-up.  Each step runs in a child process under its own
time limit, and the tool stops at the first step that fails.
usage: python3 tools/complaints3_time.py [--n 1024] [--out profiles/complaints3_time.json]
                                         [--ab-out profiles/complaints3_eval_ab.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.complaints_time import spread, timed  # noqa: E402

MODES = ((0, "auto"), (1, "horner"), (2, "tables"))
LIMIT = 420


def counts(n):
    """Complaints against one dealer (it has n - 1 receivers to cheat), then all of 16 dealers'."""
    return sorted({min(c, n - 1) for c in (1, 16, 128, n - 1)}) + [16 * (n - 1)]


def step(n, t):
    import dkg_amd

    N = t + 1
    be = dkg_amd.Backend(0)
    be.env_init(t, n)
    rec = {"device": be.pci_bus_id(), "clock_before": be.clock_probe()}
    a, b = dkg_amd.dealer_coefficients(b"\xc9" * 32, 0, 0, n, t)
    E, A, s, sp = be.share_gen(a, b, n, n, t)
    dealers = list(range(1, 17))
    A = bytearray(A)
    for i in dealers:  # a wrong A_i0: every receiver's pair passes against E and fails against A
        A[32 * N * i:32 * N * i + 32] = E[32 * N * i:32 * N * i + 32]
    A = bytes(A)
    every = [(i, q) for i in dealers for q in range(n) if q != i]

    def inputs(pairs):
        return ([q + 1 for _, q in pairs], [i + 1 for i, _ in pairs],
                b"".join(s[32 * (i * n + q):32 * (i * n + q) + 32] for i, q in pairs),
                b"".join(sp[32 * (i * n + q):32 * (i * n + q) + 32] for i, q in pairs))

    for C in counts(n):
        acc, acd, sh, rn = inputs(every[:C])
        for mode, label in MODES:
            be.set_complaint_eval(mode)

            def run():
                v, rcn = be.complaints3_verify(n, t, acc, acd, sh, rn, E, A)
                assert v == [0] * C and sum(rcn) == len(set(acd))
            rec[f"complaints3_verify_{label}_C{C}_ms"] = timed(run, 5 if C < 2000 else 3)
        be.set_complaint_eval(0)
        if C in (1, n - 1):
            rowsE = b"".join(E[32 * N * (i - 1):32 * N * i] for i in acd)
            rowsA = b"".join(A[32 * N * (i - 1):32 * N * i] for i in acd)

            def old():
                assert be.complaint3_verify(t, acc, sh, rn, rowsE, rowsA) == [0] * C
            rec[f"complaint3_verify_C{C}_ms"] = timed(old, 3)
    rec["clock_after"] = be.clock_probe()
    be.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--ts", default="511,3", help="thresholds, the first one is compared with the primitive")
    ap.add_argument("--out", default=os.path.join("profiles", "complaints3_time.json"))
    ap.add_argument("--ab-out", default=os.path.join("profiles", "complaints3_eval_ab.txt"))
    ap.add_argument("--step", type=int, help="(internal) run threshold t in this process and write its record to --frag")
    ap.add_argument("--frag")
    args = ap.parse_args()
    if args.step is not None:
        rec = step(args.n, args.step)
        with open(args.frag, "w") as f:
            json.dump(rec, f)
        return 0
    n = args.n
    ts = [int(x) for x in args.ts.split(",")]
    out = {"n": n, "command": "python3 tools/complaints3_time.py --n %d --ts %s" % (n, args.ts)}
    with tempfile.TemporaryDirectory() as tmp:
        for t in ts:
            frag = os.path.join(tmp, "t%d.json" % t)
            cmd = [sys.executable, os.path.abspath(__file__), "--n", str(n), "--step", str(t), "--frag", frag]
            try:
                rc = subprocess.run(cmd, timeout=LIMIT).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print(f"step t={t} failed (exit {rc}); stopping", file=sys.stderr)
                return 1
            with open(frag) as f:
                out["t%d" % t] = json.load(f)
            print("t=%d" % t, json.dumps(out["t%d" % t]), flush=True)
    for t in ts:
        r = out["t%d" % t]
        for C in (1, n - 1):
            r["old_over_new_C%d" % C] = round(r[f"complaint3_verify_C{C}_ms"]["median"] /
                                              r[f"complaints3_verify_auto_C{C}_ms"]["median"], 2)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    with open(args.ab_out, "w") as f:
        f.write("# P^E_i(j) and P^A_i(j) of C round-4 complaints (C <= n - 1: against ONE dealer; 16 (n - 1): against 16):\n"
                "# per-pair Horner (mode 1) against the difference tables of the accused rows (mode 2) and the\n"
                "# automatic mode (0, complaint_tables_pay with round 1's constants); dkg_complaints3_verify call,\n"
                "# wall ms, median [min, max].  `picked`: the path the automatic mode's time sits nearer to.\n"
                "# %s\n" % out["command"])
        for t in ts:
            r = out["t%d" % t]
            f.write("n = %d, t = %d, %s\n" % (n, t, r["device"]))
            f.write("%8s %26s %26s %26s %8s\n" % ("C", "horner", "tables", "auto", "picked"))
            for C in counts(n):
                cols = [r[f"complaints3_verify_{label}_C{C}_ms"] for label in ("horner", "tables", "auto")]
                h, tb, au = (c["median"] for c in cols)
                f.write("%8d" % C + "".join(" %10.2f [%6.2f, %6.2f]" % (c["median"], c["min"], c["max"]) for c in cols))
                f.write(" %8s\n" % ("horner" if abs(au - h) < abs(au - tb) else "tables"))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
