"""Time of the seats calls (receivers.hip k_seat_horner): one operator's party index in each of S
ceremonies, one seat per ceremony with a random index, against what the operator could do before.

Steps "n64" (64, 31) and "n16" (16, 7), over S = 1, 16, 256, 1,000 and 10,000:
  (a) verify_seats (round 2) against the loop of verify_receivers, one call per seat (at S = 10,000 the
      loop is 200 calls, scaled by S / 200: "loop_scaled_from");
  (b) commitment_eval_seats against commitment_eval_pairs on the same S n (row, index) pairs;
  device phases (set_streams(1)) of verify_seats under both field multiplications and the default, and
  the lane occupancy of the packing (live lanes / 64 waves).
Step "party": party_round2_seats against the loop of party_round2 at S = 256, both sizes, with nonces and
a tampered dealer in one ceremony of the pool (a few REJECTs, so the proof stage runs).

The commitments of a pool of at most 256 generated ceremonies are repeated to make up S ceremonies: the
work does not depend on the values, and S = 10,000 at (64, 31) is still 655 MB of upload per call.
Every call is synchronous (upload, kernels, copy back): wall-clock ms, median of 5 after a warm-up, all
variants interleaved within each repetition in one process, a clock probe before and after each step.
Each step runs in a child process under its own time limit; the tool stops at the first step that fails.
usage: python3 tools/seats_time.py [--out profiles/seats_time.json] [--steps n64,n16,party]
"""
import argparse
import ctypes
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
SIZES = {"n64": (64, 31), "n16": (16, 7)}
STEPS = [("n64", 540), ("n16", 300), ("party", 300)]
SEATS = (1, 16, 256, 1000, 10000)
POOL = 256
LOOP_CAP = 200  # calls of the loop that are timed where S > 1,000
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


def pool_ceremonies(be, n, t, count, master=b"\xc7" * 32):
    """E, s, s' of `count` honest ceremonies: [count * n][t+1][32] and [count * n][n][32] (one share_gen)."""
    import dkg_amd

    a = b = b""
    for c in range(count):
        ac, bc = dkg_amd.dealer_coefficients(master, c, 0, n, t)
        a, b = a + ac, b + bc
    E, _, s, sp = be.share_gen(a, b, count * n, n, t)
    return E, s, sp


def column(mat, n, c, j):
    """[n][32]: the shares addressed to party j of ceremony c, from [count * n][n][32]."""
    return b"".join(mat[32 * ((c * n + i) * n + j):32 * ((c * n + i) * n + j) + 32] for i in range(n))


def size_step(name):
    import dkg_amd

    n, t = SIZES[name]
    be = dkg_amd.Backend(0)
    be.env_init(t, n)
    lib = dkg_amd.lib()
    rec = {"n": n, "t": t, "device": be.pci_bus_id(), "pool": POOL, "clock_before": be.clock_probe(), "rows": []}
    Ep, sp_, spp = pool_ceremonies(be, n, t, POOL)
    rowlen = 32 * n * (t + 1)
    rng = random.Random(n)
    for S in SEATS:
        pool = min(S, POOL)
        E = (Ep[:rowlen * pool] * (S // pool + 1))[:rowlen * S]
        cer = list(range(S))
        js = [rng.randrange(n) for _ in range(S)]
        sc = b"".join(column(sp_, n, c % pool, j) for c, j in zip(cer, js))
        spc = b"".join(column(spp, n, c % pool, j) for c, j in zip(cer, js))
        pk = dkg_amd.seat_pack(n, js)
        row = {"seats": S, "waves": pk["waves"], "occupancy": round(S * n / (64.0 * pk["waves"]), 4)}
        ref = be.verify_seats(S, n, t, 2, cer, js, E, sc, spc)
        assert set(ref) <= {1, 2} and ref.count(2) == S  # honest ceremonies: ACCEPT, and SELF once per seat
        # (a) the loop: one verify_receivers per seat on its ceremony's commitments
        nloop = S if S <= 1000 else LOOP_CAP
        per = [(E[rowlen * c:rowlen * (c + 1)], [js[c]], sc[32 * n * c:32 * n * (c + 1)], spc[32 * n * c:32 * n * (c + 1)])
               for c in range(nloop)]

        def loop():
            out = b"".join(be.verify_receivers(n, t, 2, j1, Ec, s1, sp1) for Ec, j1, s1, sp1 in per)
            assert out == ref[:n * nloop]

        def seats():
            assert be.verify_seats(S, n, t, 2, cer, js, E, sc, spc) == ref

        # (b) the same evaluations as S n (row, index) pairs, one wave each; arrays built once for both
        cnt = S * n
        rows_a = (ctypes.c_uint32 * cnt)(*[c * n + i for c in cer for i in range(n)])
        pjs_a = (ctypes.c_uint32 * cnt)(*[j for j in js for _ in range(n)])
        cer_a, js_a = (ctypes.c_uint32 * S)(*cer), (ctypes.c_uint32 * S)(*js)
        P1, P2 = ctypes.create_string_buffer(32 * cnt), ctypes.create_string_buffer(32 * cnt)
        ok1, ok2 = ctypes.create_string_buffer(cnt), ctypes.create_string_buffer(cnt)

        def eval_pairs():
            assert lib.dkg_commitment_eval_pairs(be.ctx, S * n, t, cnt, rows_a, pjs_a, E, P1, ok1) == 0

        def eval_seats():
            assert lib.dkg_commitment_eval_seats(be.ctx, S, n, t, S, cer_a, js_a, E, P2, ok2) == 0

        row["wall_ms"] = interleaved({"verify_seats": seats, "verify_receivers_loop": loop, "eval_seats": eval_seats,
                                      "eval_pairs": eval_pairs})
        assert P1.raw == P2.raw and ok1.raw == ok2.raw
        w = row["wall_ms"]
        scale = S / nloop
        if nloop < S:
            row["loop_scaled_from"] = nloop
        row["loop_over_seats"] = round(w["verify_receivers_loop"]["min"] * scale / w["verify_seats"]["median"], 2)
        row["pairs_over_seats"] = round(w["eval_pairs"]["min"] / w["eval_seats"]["median"], 2)
        row["one_call_below_loop"] = w["verify_seats"]["median"] < w["verify_receivers_loop"]["min"] * scale
        be.set_streams(1)  # device phases, and the kernel under both field multiplications
        for mode, tag in ((0, "default"), (1, "prodscan"), (2, "colsum")):
            be.set_field_mode(mode)
            ph = []
            for _ in range(4):
                seats()
                ph.append(be.phase_times("seats"))
            row["phase_ms_" + tag] = {k: round(statistics.median(p[k] for p in ph[1:]), 4) for k in ph[0]}
        be.set_field_mode(0)
        be.set_streams(2)
        rec["rows"].append(row)
        print(name, json.dumps(row), flush=True)
    rec["clock_after"] = be.clock_probe()
    be.close()
    return rec


def party_step():
    import dkg_amd

    S, pool = 256, 16
    out = {}
    for name, (n, t) in SIZES.items():
        be = dkg_amd.Backend(0)
        be.env_init(t, n)
        rec = {"n": n, "t": t, "seats": S, "pool": pool, "device": be.pci_bus_id(), "clock_before": be.clock_probe()}
        master = b"\xc7" * 32
        E, s, sp = pool_ceremonies(be, n, t, pool, master)
        rowlen = 32 * n * (t + 1)
        sb = bytearray(s)  # ceremony 0 of the pool: dealer 1 deals shares off by one
        for q in range(n):
            k = 32 * ((0 * n + 1) * n + q)
            sb[k:k + 32] = ((int.from_bytes(s[k:k + 32], "little") + 1) % L).to_bytes(32, "little")
        s = bytes(sb)
        keys, e1s, cts = [], [], []
        for c in range(pool):
            sk, pk = be.member_keys(master, c, n)
            e1, ct = be.encrypt_shares(pk, s[32 * n * n * c:32 * n * n * (c + 1)], sp[32 * n * n * c:32 * n * n * (c + 1)],
                                       dkg_amd.enc_randomness(master, c, 0, n, n, t), n, n)
            keys.append(sk), e1s.append(e1), cts.append(ct)
        rng = random.Random(S + n)
        cer = list(range(S))
        js = [rng.randrange(n) for _ in range(S)]
        Eall = (E * (S // pool + 1))[:rowlen * S]
        col = lambda buf, j: b"".join(buf[64 * (i * n + j):64 * (i * n + j) + 64] for i in range(n))  # noqa: E731
        e1c = [col(e1s[c % pool], j) for c, j in zip(cer, js)]
        ctc = [col(cts[c % pool], j) for c, j in zip(cer, js)]
        skc = [keys[c % pool][32 * j:32 * j + 32] for c, j in zip(cer, js)]
        wc = [b"".join(((0x9e3779b97f4a7c15 * (2 * (p * n + i) + h + 1)) % L).to_bytes(32, "little")
                       for i in range(n) for h in (0, 1)) for p in range(S)]
        e1a, cta, ska, wa = b"".join(e1c), b"".join(ctc), b"".join(skc), b"".join(wc)
        ref = be.party_round2_seats(S, n, t, cer, js, Eall, e1a, cta, ska, wa)
        rec["rejects"] = sum(ref["complaints"])
        assert rec["rejects"] > 0

        def seats():
            assert be.party_round2_seats(S, n, t, cer, js, Eall, e1a, cta, ska, wa) == ref

        def loop():
            for p in range(S):
                r = be.party_round2(n, t, js[p], Eall[rowlen * p:rowlen * (p + 1)], e1c[p], ctc[p], skc[p], wc[p])
                assert r["dec"] == ref["dec"][n * p:n * (p + 1)] and r["proofs"] == ref["proofs"][192 * n * p:192 * n * (p + 1)]

        rec["wall_ms"] = interleaved({"party_round2_seats": seats, "party_round2_loop": loop})
        w = rec["wall_ms"]
        rec["loop_over_seats"] = round(w["party_round2_loop"]["min"] / w["party_round2_seats"]["median"], 2)
        rec["one_call_below_loop"] = w["party_round2_seats"]["median"] < w["party_round2_loop"]["min"]
        be.set_streams(1)
        ph = []
        for _ in range(4):
            seats()
            ph.append(be.phase_times("seats"))
        rec["phase_ms"] = {k: round(statistics.median(p[k] for p in ph[1:]), 4) for k in ph[0]}
        be.set_streams(2)
        rec["clock_after"] = be.clock_probe()
        be.close()
        out[name] = rec
        print("party", name, json.dumps(rec), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "seats_time.json"))
    ap.add_argument("--steps", default=",".join(s for s, _ in STEPS))
    ap.add_argument("--step", help="(internal) run one step in this process and write its record to --frag")
    ap.add_argument("--frag")
    args = ap.parse_args()
    if args.step:
        rec = party_step() if args.step == "party" else size_step(args.step)
        with open(args.frag, "w") as f:
            json.dump(rec, f)
        return 0
    steps = args.steps.split(",")
    out = {"command": "python3 tools/seats_time.py --steps " + ",".join(steps)}
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
