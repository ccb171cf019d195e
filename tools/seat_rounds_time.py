"""Time of the hosted seats' rounds 3-5 against what an operator could do before: one call per ceremony.

S ceremonies of (64, 31), one seat per ceremony with a random index; steps "s1000" and "s10000":
  (a) complaints_verify_ceremonies with 63 round-2 complaints per ceremony (every other receiver against one
      cheating dealer, all proven) against one complaints_verify call per ceremony;
  (b) complaints3_verify_ceremonies with 63 round-4 complaints per ceremony (against a dealer whose A_0 was
      replaced, all valid) against one complaints3_verify call per ceremony;
  (c) finalise_seats with two reconstructed dealers per ceremony and all 62 final parties disclosing, against
      one finalise_parties call per ceremony on a share matrix filled only in the seat's column and the
      disclosed entries, its result read at the seat's party (the only route before);
  and party_round3_seats alone (it has no per-ceremony counterpart), with the device phases of finalise_seats.
Where S > 1,000 the loops are timed over 200 ceremonies and scaled by S / 200 ("loop_scaled_from").

The data of a pool of 16 generated ceremonies is repeated to make up S: the work does not depend on the
values.  Every call is synchronous: wall-clock ms, median of 3 after a warm-up, the two sides of a pair
interleaved in one process, a clock probe before and after each step.  Each step runs in a child process
under its own time limit; the tool stops at the first step that fails.
usage: python3 tools/seat_rounds_time.py [--out profiles/seat_rounds_time.json] [--steps s1000,s10000]
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
G = bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76")
N, T = 64, 31
STEPS = [("s1000", 1000, 480), ("s10000", 10000, 560)]
POOL = 16
LOOP_CAP = 200
REPS = 3
CHEAT, BAD_A, RECON = 1, 2, (2, 5)  # 0-based dealers: deals wrong shares; A_0 replaced; reconstructed in (c)


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3),
            "count": len(xs)}


def interleaved(calls, reps=REPS):
    for f in calls.values():
        f()
    wall = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    return {k: spread(v) for k, v in wall.items()}


def u32(xs):
    return (ctypes.c_uint32 * max(len(xs), 1))(*xs)


def make_pool(be):
    """POOL ceremonies with member keys: dealer CHEAT deals every share off by one (63 provable round-2
    complaints), dealer BAD_A's A_0 is replaced (63 valid round-4 complaints)."""
    import dkg_amd

    n, t, master = N, T, b"\xd3" * 32
    pool = []
    for c in range(POOL):
        a, b = dkg_amd.dealer_coefficients(master, c, 0, n, t)
        E, A, s, sp = be.share_gen(a, b, n, n, t)
        sb = bytearray(s)
        for q in range(n):
            k = 32 * (CHEAT * n + q)
            sb[k:k + 32] = ((int.from_bytes(s[k:k + 32], "little") + 1) % L).to_bytes(32, "little")
        sent = bytes(sb)
        k = 32 * (t + 1) * BAD_A
        A = A[:k] + G + A[k + 32:]
        sk, pk = be.member_keys(master, c, n)
        e1, ct = be.encrypt_shares(pk, sent, sp, dkg_amd.enc_randomness(master, c, 0, n, n, t), n, n)
        acc = [q for q in range(n) if q != CHEAT]
        enc = b"".join(e1[64 * (CHEAT * n + q):64 * (CHEAT * n + q) + 32] + ct[64 * (CHEAT * n + q):64 * (CHEAT * n + q) + 32]
                       + e1[64 * (CHEAT * n + q) + 32:64 * (CHEAT * n + q) + 64]
                       + ct[64 * (CHEAT * n + q) + 32:64 * (CHEAT * n + q) + 64] for q in acc)
        w = b"".join(((0x9e3779b97f4a7c15 * (2 * (c * n + q) + h + 1)) % L).to_bytes(32, "little")
                     for q in acc for h in (0, 1))
        proofs = be.complaints_prove(b"".join(sk[32 * q:32 * q + 32] for q in acc), enc, w)
        acc4 = [q for q in range(n) if q != BAD_A]
        pool.append(dict(E=E, A=A, s=sent, pk=pk, acc2=[q + 1 for q in acc], enc=enc, proofs=proofs,
                         acc4=[q + 1 for q in acc4],
                         share4=b"".join(sent[32 * (BAD_A * n + q):32 * (BAD_A * n + q) + 32] for q in acc4),
                         rand4=b"".join(sp[32 * (BAD_A * n + q):32 * (BAD_A * n + q) + 32] for q in acc4),
                         A0=b"".join(A[32 * (t + 1) * i:32 * (t + 1) * i + 32] for i in range(n))))
    return pool


def size_step(S):
    import dkg_amd

    n, t = N, T
    be = dkg_amd.Backend(0)
    be.env_init(t, n)
    lib = dkg_amd.lib()
    rec = {"n": n, "t": t, "seats": S, "pool": POOL, "device": be.pci_bus_id(), "clock_before": be.clock_probe()}
    pool = make_pool(be)
    nloop = S if S <= 1000 else LOOP_CAP
    scale = S / nloop
    if nloop < S:
        rec["loop_scaled_from"] = nloop
    rep = lambda key: b"".join(pool[c % POOL][key] for c in range(S))  # noqa: E731
    rng = random.Random(S)
    cer, js = list(range(S)), [rng.randrange(n) for _ in range(S)]
    cer_a, js_a = u32(cer), u32(js)
    E, A, pk = rep("E"), rep("A"), rep("pk")

    def below(w, one, loop):
        return {"loop_over_one_call": round(w[loop]["min"] * scale / w[one]["median"], 2),
                "one_call_below_loop": w[one]["median"] < w[loop]["min"] * scale}

    # ---- (a) round-2 complaints
    C = 63 * S
    ceremony = u32([c for c in range(S) for _ in range(63)])
    accuser = u32([q for c in range(S) for q in pool[c % POOL]["acc2"]])
    accused = u32([CHEAT + 1] * C)
    enc, proofs = rep("enc"), rep("proofs")
    verdict, qual = (ctypes.c_int32 * C)(), ctypes.create_string_buffer(S * n)

    def c2_one():
        assert lib.dkg_complaints_verify_ceremonies(be.ctx, S, n, t, C, ceremony, accuser, accused, pk, E, None, enc,
                                                    proofs, verdict, qual) == 0

    def c2_loop():
        for c in range(nloop):
            p = pool[c % POOL]
            v, q = be.complaints_verify(n, t, p["acc2"], [CHEAT + 1] * 63, p["pk"], p["E"], p["enc"], p["proofs"])
            assert v == [0] * 63 and q == [int(i != CHEAT) for i in range(n)]

    w = interleaved({"complaints_verify_ceremonies": c2_one, "complaints_verify_loop": c2_loop})
    assert list(verdict) == [0] * C and qual.raw == bytes(int(i != CHEAT) for i in range(n)) * S
    rec["round2_complaints"] = dict(complaints=C, wall_ms=w,
                                    **below(w, "complaints_verify_ceremonies", "complaints_verify_loop"))
    print(S, "round2", json.dumps(rec["round2_complaints"]), flush=True)

    # ---- (b) round-4 complaints
    accuser4 = u32([q for c in range(S) for q in pool[c % POOL]["acc4"]])
    accused4 = u32([BAD_A + 1] * C)
    share4, rand4 = rep("share4"), rep("rand4")
    recon = ctypes.create_string_buffer(S * n)

    def c4_one():
        assert lib.dkg_complaints3_verify_ceremonies(be.ctx, S, n, t, C, ceremony, accuser4, accused4, share4, rand4, E, A,
                                                     None, None, verdict, recon) == 0

    def c4_loop():
        for c in range(nloop):
            p = pool[c % POOL]
            v, r = be.complaints3_verify(n, t, p["acc4"], [BAD_A + 1] * 63, p["share4"], p["rand4"], p["E"], p["A"])
            assert v == [0] * 63 and r == [int(i == BAD_A) for i in range(n)]

    w = interleaved({"complaints3_verify_ceremonies": c4_one, "complaints3_verify_loop": c4_loop})
    assert list(verdict) == [0] * C and recon.raw == bytes(int(i == BAD_A) for i in range(n)) * S
    rec["round4_complaints"] = dict(complaints=C, wall_ms=w,
                                    **below(w, "complaints3_verify_ceremonies", "complaints3_verify_loop"))
    print(S, "round4", json.dumps(rec["round4_complaints"]), flush=True)

    # ---- (c) finalise: two reconstructed dealers, every final party discloses
    q1 = bytes([1] * n)
    r1 = bytes(int(i in RECON) for i in range(n))
    final = [q for q in range(n) if q not in RECON]
    col = lambda c, j: b"".join(pool[c % POOL]["s"][32 * (i * n + j):32 * (i * n + j) + 32] for i in range(n))  # noqa: E731
    cols = b"".join(col(c, j) for c, j in zip(cer, js))
    A0 = rep("A0")
    d_cer = u32([c for c in range(S) for _ in RECON for _ in final])
    d_snd = u32([q + 1 for _ in range(S) for _ in RECON for q in final])
    d_dlr = u32([i + 1 for _ in range(S) for i in RECON for _ in final])
    d_one = [b"".join(p["s"][32 * (i * n + q):32 * (i * n + q) + 32] for i in RECON for q in final) for p in pool]
    d_sh = b"".join(d_one[c % POOL] for c in range(S))
    D5 = len(final) * len(RECON) * S
    mpk, status, index = ctypes.create_string_buffer(32 * S), (ctypes.c_int32 * S)(), (ctypes.c_int32 * S)()
    qS, rS = q1 * S, r1 * S

    def fin_one():
        assert lib.dkg_finalise_seats(be.ctx, S, n, t, S, cer_a, js_a, qS, rS, None, None, None, A0, cols, D5, d_cer,
                                      d_snd, d_dlr, d_sh, mpk, status, index) == 0

    mats = []
    for c in range(nloop):  # the share matrix an operator can fill: its own column and the disclosed rows
        p, j = pool[c % POOL], js[c]
        m = bytearray(32 * n * n)
        for i in range(n):
            m[32 * (i * n + j):32 * (i * n + j) + 32] = p["s"][32 * (i * n + j):32 * (i * n + j) + 32]
        for i in RECON:
            m[32 * i * n:32 * (i + 1) * n] = p["s"][32 * i * n:32 * (i + 1) * n]
        mats.append(bytes(m))
    got = []

    def fin_loop():
        got.clear()
        for c in range(nloop):
            pf = be.finalise_parties(n, t, q1, r1, pool[c % POOL]["A0"], mats[c])
            assert pf.status[js[c]] == 0
            got.append(pf.mpk[js[c]])

    def r3_one():
        be.party_round3_seats(S, n, t, cer, js, qS, cols)

    w = interleaved({"finalise_seats": fin_one, "finalise_parties_loop": fin_loop, "party_round3_seats": r3_one})
    assert list(status) == [0] * S and b"".join(got) == mpk.raw[:32 * nloop]
    rec["finalise"] = dict(disclosures=D5, wall_ms=w, **below(w, "finalise_seats", "finalise_parties_loop"))
    be.set_streams(1)
    ph = []
    for _ in range(4):
        fin_one()
        ph.append(be.phase_times("seats"))
    rec["finalise"]["phase_ms"] = {k: round(statistics.median(p[k] for p in ph[1:]), 4) for k in ("lagrange", "mpk")}
    be.set_streams(2)
    print(S, "finalise", json.dumps(rec["finalise"]), flush=True)
    rec["clock_after"] = be.clock_probe()
    be.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "seat_rounds_time.json"))
    ap.add_argument("--steps", default=",".join(s for s, _, _ in STEPS))
    ap.add_argument("--step", help="(internal) run one step in this process and write its record to --frag")
    ap.add_argument("--frag")
    args = ap.parse_args()
    if args.step:
        rec = size_step({s: S for s, S, _ in STEPS}[args.step])
        with open(args.frag, "w") as f:
            json.dump(rec, f)
        return 0
    steps = args.steps.split(",")
    out = {"command": "python3 tools/seat_rounds_time.py --steps " + ",".join(steps)}
    if os.path.exists(args.out):  # steps run in several visits accumulate in one record
        with open(args.out) as f:
            out.update({k: v for k, v in json.load(f).items() if k != "command"})
    with tempfile.TemporaryDirectory() as tmp:
        for name, _, limit in STEPS:
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
