"""Time of the batched complaint verification (dkg_complaints_verify) at n = 1024, t = 511, against the
host-driven primitive it stands beside (dkg_complaint1_verify), the A/B of its two evaluations of
P_i(j) (per-pair Horner against the difference tables of the accused row), and the full-mode ceremony
with and without the complaints.

Every call here is synchronous (uploads, kernels, the copy back), so the figures are wall-clock
milliseconds of the call, medians after a warm-up.  Each step runs in a child process under its own
time limit, and the tool stops at the first step that fails.
usage: python3 tools/complaints_time.py [--n 1024] [--t 511] [--out profiles/complaints_time.json]
                                        [--ab-out profiles/complaints_eval_ab.txt]
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
sys.path.insert(0, ROOT)
L = 2**252 + 27742317777372353535851937790883648493
STEPS = [("new", 420), ("old", 300), ("ab", 420), ("ceremony", 300)]


def ab_counts(n):
    """Complaints against one dealer in the evaluation A/B (a dealer has n - 1 receivers to cheat)."""
    return sorted({min(c, n - 1) for c in (1, 16, 128, n - 1)})


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3),
            "count": len(xs)}


def timed(f, reps):
    f()  # warm-up: allocations, code objects
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        out.append((time.perf_counter() - t0) * 1e3)
    return spread(out)


def committee(be, n, t, cheats):
    """A seeded full-mode committee in which the dealers `cheats` (0-based) send every other receiver
    a wrong share: (E, A, e1, ct, sk, pk)."""
    import dkg_amd

    master = b"\xc7" * 32
    a, b = dkg_amd.dealer_coefficients(master, 0, 0, n, t)
    E, A, s, sp = be.share_gen(a, b, n, n, t)
    s = bytearray(s)
    for i in cheats:
        for q in range(n):
            if q != i:
                k = 32 * (i * n + q)
                s[k:k + 32] = ((int.from_bytes(s[k:k + 32], "little") + 1) % L).to_bytes(32, "little")
    sk, pk = be.member_keys(master, 0, n)
    e1, ct = be.encrypt_shares(pk, bytes(s), sp, dkg_amd.enc_randomness(master, 0, 0, n, n, t), n, n)
    return E, A, e1, ct, sk, pk


def complaints(be, n, e1, ct, sk, pairs):
    """Honest proofs (on the device) of the receivers' complaints `pairs` [(dealer, receiver)], 0-based."""
    def enc_of(i, q):
        k = 2 * (i * n + q)
        return e1[32 * k:32 * k + 32] + ct[32 * k:32 * k + 32] + e1[32 * k + 32:32 * k + 64] + ct[32 * k + 32:32 * k + 64]

    enc = b"".join(enc_of(i, q) for i, q in pairs)
    w = b"".join(((0x9e3779b97f4a7c15 * (c + 1)) % L).to_bytes(32, "little") for c in range(2 * len(pairs)))
    proofs = be.complaints_prove(b"".join(sk[32 * q:32 * q + 32] for _, q in pairs), enc, w)
    return [q + 1 for _, q in pairs], [i + 1 for i, _ in pairs], enc, proofs


def step(name, n, t):
    import dkg_amd

    N = t + 1
    be = dkg_amd.Backend(0)
    be.env_init(t, n)
    rec = {"device": be.pci_bus_id(), "clock_before": be.clock_probe()}
    dealers = list(range(1, 17)) if name == "new" else [1]
    E, A, e1, ct, sk, pk = committee(be, n, t, dealers)
    every = [(i, q) for i in dealers for q in range(n) if q != i]

    def verify(pairs, mode):
        acc, acd, enc, proofs = complaints(be, n, e1, ct, sk, pairs)
        be.set_complaint_eval(mode)

        def run():
            v, q = be.complaints_verify(n, t, acc, acd, pk, E, enc, proofs)
            assert v == [0] * len(pairs) and sum(q) == n - len({i for i, _ in pairs})
        return run

    if name == "new":
        for C in (1, n - 1, 16 * (n - 1)):
            rec[f"complaints_verify_C{C}_ms"] = timed(verify(every[:C], 0), 5 if C < 2000 else 3)
    elif name == "old":
        for C in (1, n - 1):
            acc, acd, enc, proofs = complaints(be, n, e1, ct, sk, every[:C])
            pks = b"".join(pk[32 * (q - 1):32 * q] for q in acc)
            rows = b"".join(E[32 * N * (i - 1):32 * N * i] for i in acd)

            def run():
                assert be.complaint1_verify(t, acc, pks, enc, rows, proofs) == [0] * C
            rec[f"complaint1_verify_C{C}_ms"] = timed(run, 3)
    elif name == "ab":
        for C in ab_counts(n):
            for mode, label in ((1, "horner"), (2, "tables")):
                rec[f"eval_{label}_C{C}_ms"] = timed(verify(every[:C], mode), 5)
    elif name == "ceremony":
        acc, acd, enc, proofs = complaints(be, n, e1, ct, sk, every)
        dev, wall = {"plain": [], "complaints": []}, {"plain": [], "complaints": []}
        for rep in range(4):
            t0 = time.perf_counter()
            r = be.ceremony_verify_full(E, A, e1, ct, sk, n, t)
            t1 = time.perf_counter()
            rc, v, dis = be.ceremony_verify_full_complaints(E, A, e1, ct, sk, pk, acc, acd, proofs, n, t)
            t2 = time.perf_counter()
            assert v == [0] * len(acc) and dis == [0] * n and rc.qualified == r.qualified and rc.mpk == r.mpk
            if rep:  # the first pass allocates
                dev["plain"].append(r.ms["total"])
                dev["complaints"].append(rc.ms["total"])
                wall["plain"].append((t1 - t0) * 1e3)
                wall["complaints"].append((t2 - t1) * 1e3)
        rec["ceremony_verify_full"] = {"device_ms": spread(dev["plain"]), "wall_ms": spread(wall["plain"])}
        rec["ceremony_verify_full_complaints"] = {"complaints": len(acc), "rounds_device_ms": spread(dev["complaints"]),
                                                  "wall_ms": spread(wall["complaints"])}
    rec["clock_after"] = be.clock_probe()
    be.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--t", type=int, default=511)
    ap.add_argument("--out", default=os.path.join("profiles", "complaints_time.json"))
    ap.add_argument("--ab-out", default=os.path.join("profiles", "complaints_eval_ab.txt"))
    ap.add_argument("--steps", default=",".join(s for s, _ in STEPS))
    ap.add_argument("--step", help="(internal) run one step in this process and write its record to --frag")
    ap.add_argument("--frag")
    args = ap.parse_args()
    if args.step:
        rec = step(args.step, args.n, args.t)
        with open(args.frag, "w") as f:
            json.dump(rec, f)
        return 0
    out = {"n": args.n, "t": args.t, "command": "python3 tools/complaints_time.py --n %d --t %d" % (args.n, args.t)}
    with tempfile.TemporaryDirectory() as tmp:
        for name, limit in STEPS:
            if name not in args.steps.split(","):
                continue
            frag = os.path.join(tmp, name + ".json")
            cmd = [sys.executable, os.path.abspath(__file__), "--n", str(args.n), "--t", str(args.t), "--step", name,
                   "--frag", frag]
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
    if "new" in out and "old" in out:
        C = args.n - 1
        out["old_over_new_C%d" % C] = round(out["old"][f"complaint1_verify_C{C}_ms"]["median"] /
                                            out["new"][f"complaints_verify_C{C}_ms"]["median"], 2)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    if "ab" in out:
        with open(args.ab_out, "w") as f:
            f.write("# P_i(j) of C complaints against ONE dealer: per-pair Horner (mode 1) against the difference\n"
                    "# tables of its row (mode 2); dkg_complaints_verify call, wall ms, median [min, max] of 5\n"
                    "# %s --steps ab   (n = %d, t = %d, %s)\n" % (out["command"], args.n, args.t, out["ab"]["device"]))
            f.write("%8s %28s %28s\n" % ("C", "horner", "tables"))
            for C in ab_counts(args.n):
                h, tb = out["ab"][f"eval_horner_C{C}_ms"], out["ab"][f"eval_tables_C{C}_ms"]
                f.write("%8d %12.2f [%6.2f, %6.2f] %12.2f [%6.2f, %6.2f]\n" % (C, h["median"], h["min"], h["max"],
                                                                             tb["median"], tb["min"], tb["max"]))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
