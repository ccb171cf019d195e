"""Time of a batch of full-mode ceremonies decided by the PROVEN complaints
(dkg_ceremony_batch_verify_full_proven), against the same inputs through dkg_ceremony_batch_verify_full
(the rejection rule: what the complaint stages add) and through a loop of one
dkg_ceremony_verify_full_proven call per ceremony (the only other route to the same outputs).

Every ceremony has one dealer that encrypts wrong shares to all others (n - 1 round-1 complaints, proved
with dkg_complaints_prove) and one dealer with a wrong A_0 (n - 1 round-4 complaints).  All three routes
take host arrays, so their wall times include the upload of the broadcasts.
usage: python3 tools/batch_proven_time.py --B 1000 --n 64 --t 31 [--steps 5] [--loop 1000]
                                          [--out profiles/batch_proven_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

L = 2**252 + 27742317777372353535851937790883648493


def sc(v):
    return (v % L).to_bytes(32, "little")


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "mean": round(statistics.fmean(xs), 4), "min": round(min(xs), 4),
            "max": round(max(xs), 4), "count": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1000)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--t", type=int, default=31)
    ap.add_argument("--steps", type=int, default=5, help="timed calls of each batch route")
    ap.add_argument("--loop", type=int, default=0, help="ceremonies of the one-call-per-ceremony loop (0: all B)")
    ap.add_argument("--loop-steps", type=int, default=3, help="timed passes of the loop")
    ap.add_argument("--out", default=os.path.join("profiles", "batch_proven_time.json"))
    args = ap.parse_args()
    import torch

    import dkg_amd
    from dkg_amd import _lib

    B, n, t = args.B, args.n, args.t
    N, V = t + 1, args.B * args.n
    master = b"\xc3" * 32
    dev = torch.device("cuda", 0)
    be = dkg_amd.Backend(0)
    be.env_init(t, n)
    # ---- inputs (untimed): B honest ceremonies, then the two faults of each
    coeffs = [dkg_amd.dealer_coefficients(master, c, 0, n, t) for c in range(B)]
    a, b = b"".join(x[0] for x in coeffs), b"".join(x[1] for x in coeffs)
    E, A, s, sp = be.share_gen(a, b, V, n, t)
    sk, pk = be.member_keys_batch(master, 0, B, n)
    tr = torch.empty(64 * V * n, dtype=torch.uint8, device=dev)
    be.enc_randomness_device(master, 0, B, 0, n, n, t, tr.data_ptr())
    r_enc = bytes(tr.cpu().numpy())
    del tr
    d2, d4 = 5 % n, 17 % n  # the dealer with wrong ciphertexts, the dealer with a wrong A_0
    sent = bytearray(s)
    for c in range(B):
        for q in range(n):
            if q != d2:
                k = 32 * ((c * n + d2) * n + q)
                sent[k:k + 32] = sc(int.from_bytes(sent[k:k + 32], "little") + 1)
    e1, ct = be.encrypt_shares_batch(pk, bytes(sent), sp, r_enc, B, n)
    del r_enc
    wrong = be.fixed_base_batch(sc(777))
    A = bytearray(A)
    for c in range(B):
        k = 32 * N * (c * n + d4)
        A[k:k + 32] = wrong
    A = bytes(A)

    def enc_of(c, i, q):
        k = 32 * 2 * ((c * n + i) * n + q)
        return e1[k:k + 32] + ct[k:k + 32] + e1[k + 32:k + 64] + ct[k + 32:k + 64]

    cer2 = [c for c in range(B) for q in range(n) if q != d2]
    acc2 = [q + 1 for c in range(B) for q in range(n) if q != d2]
    acd2 = [d2 + 1] * len(acc2)
    t0 = time.perf_counter()
    proofs = be.complaints_prove(b"".join(sk[32 * (c * n + q - 1):32 * (c * n + q)] for c, q in zip(cer2, acc2)),
                                 b"".join(enc_of(c, d2, q - 1) for c, q in zip(cer2, acc2)),
                                 b"".join(sc(2 * k + 1) + sc(2 * k + 2) for k in range(len(acc2))))
    prove_s = time.perf_counter() - t0
    cer4 = [c for c in range(B) for q in range(n) if q != d4]
    acc4 = [q + 1 for c in range(B) for q in range(n) if q != d4]
    acd4 = [d4 + 1] * len(acc4)
    at = [32 * ((c * n + d4) * n + q - 1) for c, q in zip(cer4, acc4)]
    sh4 = b"".join(s[k:k + 32] for k in at)  # what the receivers decrypt: dealer d4 encrypted its true shares
    rn4 = b"".join(sp[k:k + 32] for k in at)
    rec = {"B": B, "n": n, "t": t, "device": be.pci_bus_id(), "C": len(acc2), "C4": len(acc4),
           "complaints_prove_s": round(prove_s, 3), "clock_before": be.clock_probe()}

    def phase(name):
        return _lib.lib().dkg_ctx_phase_ms(be.ctx, name)

    # ---- the batch by proven complaints
    def proven():
        w0 = time.perf_counter()
        r = dkg_amd.ceremony_batch_verify_full_proven(be, B, n, t, E, A, e1, ct, sk, pk, cer2, acc2, acd2, proofs, cer4,
                                                      acc4, acd4, sh4, rn4)
        return r, (time.perf_counter() - w0) * 1e3

    r, _ = proven()  # warm-up: allocations, code objects
    assert r.verdict == [0] * len(acc2) and r.verdict4 == [0] * len(acc4), "a complaint of the benchmark did not hold"
    assert r.result.n_qualified == [n - 1] * B and r.finalise_status == [0] * B
    assert all(r.result.reconstruct[c * n + d4] == 1 for c in range(B))
    walls, dev_ms, c2, c4 = [], [], [], []
    for _ in range(args.steps):
        r, wall = proven()
        walls.append(wall)
        dev_ms.append(r.result.ms["total"])
        c2.append(phase(b"bproven.c2"))
        c4.append(phase(b"bproven.c4"))
    rec["batch_proven"] = {"wall_ms": spread(walls), "rounds_device_ms": spread(dev_ms), "bproven_c2_ms": spread(c2),
                           "bproven_c4_ms": spread(c4)}
    keep = r

    # ---- the same inputs under the rejection rule: no complaint stage
    dkg_amd.ceremony_batch_verify_full(be, B, n, t, E, A, e1, ct, sk)
    walls_r, dev_r = [], []
    for _ in range(args.steps):
        w0 = time.perf_counter()
        rr = dkg_amd.ceremony_batch_verify_full(be, B, n, t, E, A, e1, ct, sk)
        walls_r.append((time.perf_counter() - w0) * 1e3)
        dev_r.append(rr.ms["total"])
    rec["batch_rejection"] = {"wall_ms": spread(walls_r), "rounds_device_ms": spread(dev_r)}
    rec["complaint_stages_add_wall_ms"] = round(statistics.median(walls) - statistics.median(walls_r), 3)

    # ---- one single-ceremony call per ceremony
    loop = min(args.loop or B, B)
    per2, per4 = n - 1, n - 1
    passes = []
    for rep in range(args.loop_steps + 1):  # the first pass warms the single path's buffers
        w0 = time.perf_counter()
        for c in range(loop):
            v, v4 = slice(c * n, (c + 1) * n), slice(c * per4, (c + 1) * per4)
            v2 = slice(c * per2, (c + 1) * per2)
            one = be.ceremony_verify_full_proven(
                E[32 * N * n * c:32 * N * n * (c + 1)], A[32 * N * n * c:32 * N * n * (c + 1)],
                e1[64 * n * n * c:64 * n * n * (c + 1)], ct[64 * n * n * c:64 * n * n * (c + 1)], sk[32 * v.start:32 * v.stop],
                pk[32 * v.start:32 * v.stop], acc2[v2], acd2[v2], proofs[192 * v2.start:192 * v2.stop], acc4[v4], acd4[v4],
                sh4[32 * v4.start:32 * v4.stop], rn4[32 * v4.start:32 * v4.stop], n, t)
            if rep == 0 and c in (0, loop - 1):
                assert one.result.mpk == keep.result.mpk[c] and one.verdict == [0] * per2
        if rep:
            passes.append((time.perf_counter() - w0) * 1e3 * B / loop)
    rec["single_loop"] = {"ceremonies": loop, "wall_ms_scaled_to_B": spread(passes)}
    rec["loop_over_batch_wall"] = round(statistics.median(passes) / statistics.median(walls), 2)
    rec["clock_after"] = be.clock_probe()
    be.close()
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
