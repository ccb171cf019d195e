"""Per-rank device time of the dealer-sharded ceremony in full (encrypted-share) mode at N ranks,
emulated on ONE GPU as tools/shard_time.py does: rank 0 of an N-way split owns dealers [0, n/N) and
dkg_ceremony_shard_full_device runs exactly what that rank runs.

Per N, the device ms of the call in the four key-comb configurations of dkg_ctx_set_key_comb --
  a  radix 2^10 tables, cached        b  radix 2^10 tables, cold (keys the context has not seen)
  c  radix-16 combs, cold             d  radix-16 combs, cached
-- the plaintext shard (dkg_ceremony_shard_device) beside them, and the full.* phases of a serialised
run of each kind.  At --compose-ws (8) the call is also compared, wall time, with the only route to the
same work without it: dkg_ceremony_shard_device + dkg_encrypt_shares + dkg_decrypt_shares on the rank's
rows (host round trips for the shares and ciphertexts), keys cold and warm, interleaved.
A second, small committee (--small) gives the builds' second point: the cost rule's constants
(runtime.hip dkg_key_comb_choice) are fitted from the two ("fit": build = floor + per key).
usage: python3 tools/shard_full_time.py [n t] [--ws 1,2,4,8] [--small 64,31] [--reps 5]
                                        [--out profiles/shard_full_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHASES = ("enc_mul", "enc_encode", "enc_sym", "dec_decode", "dec_mul", "dec_encode", "dec_sym")
MASTER = b"\xbd" * 32


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3),
            "count": len(xs)}


def shape(be, n, t, ranks, compose_ws, reps):
    """The rows of one committee size, {str(ranks): row}."""
    import torch

    from dkg_amd import _lib

    N = t + 1
    u8 = dict(dtype=torch.uint8, device=torch.device("cuda", 0))
    be.env_init(t, n)
    nkeys = 2 * reps + 4
    keys = [be.member_keys(bytes([0xc0 + i]) * 32, 0, n) for i in range(nkeys)]  # distinct sets: cold builds
    fresh = iter(range(1, 10**6))
    rows = {}

    def new_keys():
        """A key set no cache of the context holds (the caches keep one set per kind)."""
        return keys[next(fresh) % (nkeys - 1) + 1]

    for ws in ranks:
        D = n // ws
        ta, tb = torch.empty(32 * D * N, **u8), torch.empty(32 * D * N, **u8)
        tr = torch.empty(64 * D * n, **u8)
        be.dealer_coefficients_device(MASTER, 0, 1, 0, D, t, ta.data_ptr(), tb.data_ptr())
        be.enc_randomness_device(MASTER, 0, 1, 0, D, n, t, tr.data_ptr())
        o2, o4 = torch.empty(D * n, **u8), torch.empty(D * n, **u8)
        oA, op = torch.empty(D * 32, **u8), torch.empty(n * 32, **u8)
        outs = (o2.data_ptr(), o4.data_ptr(), oA.data_ptr(), op.data_ptr())

        def full(kp):
            w0 = time.perf_counter()
            ms = be.ceremony_shard_full_device(n, t, 0, D, ta.data_ptr(), tb.data_ptr(), tr.data_ptr(), kp[0], kp[1],
                                               *outs)
            return ms, (time.perf_counter() - w0) * 1e3

        def plain():
            return be.ceremony_shard_device(n, t, 0, D, ta.data_ptr(), tb.data_ptr(), *outs)

        row = {"dealers": D, "items_per_key": 2 * D}
        be.set_streams(2)
        plain()
        row["plain_ms"] = spread([plain() for _ in range(reps)])
        for mode in (1, 2):  # warm both kinds' buffers
            be.set_key_comb(mode)
            full(keys[0])
        assert bool((o2.view(D, n) != 0).all()), "an honest shard rejected a decrypted share"
        cfg = {"a_cached10": [], "b_cold10": [], "c_cold16": [], "d_cached16": []}
        for _ in range(reps):  # interleaved, so that drift hits every configuration alike
            be.set_key_comb(1)
            full(keys[0])
            cfg["a_cached10"].append(full(keys[0])[0])
            cfg["b_cold10"].append(full(new_keys())[0])
            be.set_key_comb(2)
            cfg["c_cold16"].append(full(new_keys())[0])
            full(keys[0])
            cfg["d_cached16"].append(full(keys[0])[0])
        row["device_ms"] = {k: spread(v) for k, v in cfg.items()}
        be.set_key_comb(0)
        full(new_keys())
        row["mode0_cold_kind"] = be.last_key_comb()
        # serialised runs: the hybrid kernels' own times, per kind (keys cached)
        be.set_streams(1)
        row["phases_ms"] = {}
        for mode, name in ((1, "radix2^10"), (2, "radix16")):
            be.set_key_comb(mode)
            full(keys[0])
            ph = []
            for _ in range(3):
                full(keys[0])
                ph.append({p: _lib.lib().dkg_ctx_phase_ms(be.ctx, ("full." + p).encode()) for p in PHASES})
            row["phases_ms"][name] = {p: round(statistics.median(x[p] for x in ph), 4) for p in PHASES}
        be.set_streams(2)
        be.set_key_comb(0)

        if ws == compose_ws:
            # the same work without the new call: plaintext shard + host-buffer encryption and decryption
            a, b, r = (bytes(x.cpu().numpy()) for x in (ta, tb, tr))
            _, _, s, sp = be.share_gen(a, b, D, n, t)

            def compose(kp):
                w0 = time.perf_counter()
                plain()
                e1, ct = be.encrypt_shares(kp[1], s, sp, r, D, n)
                be.decrypt_shares(kp[0], e1, ct, D, n)
                return (time.perf_counter() - w0) * 1e3

            compose(keys[0])
            full(keys[0])
            w = {"compose_warm": [], "compose_cold": [], "call_warm": [], "call_cold": []}
            kinds = {}
            for _ in range(reps):
                compose(keys[0])
                w["compose_warm"].append(compose(keys[0]))
                w["compose_cold"].append(compose(new_keys()))
                full(keys[0])
                w["call_warm"].append(full(keys[0])[1])
                kinds["warm"] = be.last_key_comb()
                w["call_cold"].append(full(new_keys())[1])
                kinds["cold"] = be.last_key_comb()
            row["wall_ms_vs_composition"] = {k: spread(v) for k, v in w.items()}
            row["wall_ms_vs_composition"]["call_kinds_mode0"] = kinds
        rows[str(ws)] = row
        print(json.dumps({"n": n, "ws": ws, **row}), flush=True)
    return rows


def fit(n, big, build_row, ns, small):
    """build(keys) = floor + per_key * keys through the two committees' cold - cached differences (the
    large committee's smallest shard, where the side stream hides least of a build and the difference is
    the largest share of the call; the small committee whole); the multiplications per item from the
    large committee's largest shard, serialised enc_mul."""
    def delta(row, cold, cached):
        return (row["device_ms"][cold]["median"] - row["device_ms"][cached]["median"]) * 1e3  # us

    out = {}
    for kind, cold, cached in (("10", "b_cold10", "a_cached10"), ("16", "c_cold16", "d_cached16")):
        hi, lo = delta(build_row, cold, cached), delta(small, cold, cached)
        per = (hi - lo) / (n - ns)
        out["build%s_us_per_key" % kind] = round(per, 3)
        out["build%s_floor_us" % kind] = round(lo - per * ns, 1)
    items = 2 * big["dealers"] * n
    out["mul10_ns_per_item"] = round(big["phases_ms"]["radix2^10"]["enc_mul"] * 1e6 / items, 3)
    out["mul16_ns_per_item"] = round(big["phases_ms"]["radix16"]["enc_mul"] * 1e6 / items, 3)
    out["note"] = ("build: two-point fit over n = %d (all dealers) and n = %d (shard of %d dealers); mul: the "
                   "serialised full.enc_mul phase (e1 = g r and K = pk r together) per item at n = %d, %d dealers"
                   % (ns, n, build_row["dealers"], n, big["dealers"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int, nargs="?", default=1024)
    ap.add_argument("t", type=int, nargs="?", default=511)
    ap.add_argument("--ws", default="1,2,4,8")
    ap.add_argument("--small", default="64,31", help="n,t of the builds' second point ('' skips it and the fit)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--compose-ws", type=int, default=8, help="rank count of the comparison with the composition (0: skip)")
    ap.add_argument("--out", default=os.path.join("profiles", "shard_full_time.json"))
    args = ap.parse_args()
    import dkg_amd

    be = dkg_amd.Backend(0)
    rec = {"n": args.n, "t": args.t, "device": be.pci_bus_id(), "reps": args.reps, "clock_before": be.clock_probe()}
    rec["ranks"] = shape(be, args.n, args.t, [int(x) for x in args.ws.split(",")], args.compose_ws, args.reps)
    if args.small:
        ns, ts = (int(x) for x in args.small.split(","))
        rec["small"] = {"n": ns, "t": ts, "ranks": shape(be, ns, ts, [1], 0, args.reps)}
        order = sorted(rec["ranks"], key=int)
        rec["fit"] = fit(args.n, rec["ranks"][order[0]], rec["ranks"][order[-1]], ns, rec["small"]["ranks"]["1"])
    rec["committed_constants"] = dkg_amd.api.key_comb_constants()
    rec["clock_after"] = be.clock_probe()
    be.close()
    print(json.dumps({"fit": rec.get("fit")}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
