"""Device time of the comb-table builds under the two builders of dkg_ctx_set_comb_build -- 1 = one
thread per entry (k_build_combw, the baseline), 2 = chained (comb_build.hip) -- in one process, the
modes interleaved round by round, the clock probe before and after.

Per mode, dkg_ctx_last_comb_build_ms of: one base of the shared geometry (dkg_env_init under a fresh
commitment key) and 64 / 1,024 / 4,096 member keys of the key geometry (dkg_encrypt_shares with one
dealer row, radix-2^10 key combs forced, a fresh key set).  Then wall and device time of the setup a
ceremony under fresh keys pays: dkg_ctx_create (automatic mode), dkg_env_init, and the first full-mode
n = 1024 ceremony on fresh member keys (its device total and wall time), beside the warm ceremony.
usage: python3 tools/comb_build_time.py [--rounds 6] [--n 1024 --t 511] [--out profiles/comb_build_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MASTER = b"\xcb" * 32
MODES = (1, 2)


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4),
            "count": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--t", type=int, default=511)
    ap.add_argument("--keys", default="64,1024,4096")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    import dkg_amd

    n, t, N = args.n, args.t, args.t + 1
    key_counts = [int(x) for x in args.keys.split(",")]
    w0 = time.perf_counter()
    be = dkg_amd.Backend(0)
    create = {"wall_ms": round((time.perf_counter() - w0) * 1e3, 3), "builder": be.last_comb_build(),
              "comb_device_ms": round(be.last_comb_build_ms(), 4)}
    res = {"geometry": {str(k): dkg_amd.comb_geometry(k) for k in (0, 1)}, "rounds": args.rounds,
           "clock_before": be.clock_probe(), "ctx_create_automatic": create}
    fresh = iter(range(1, 10**6))

    def env_init(nn, tt):
        """dkg_env_init under a commitment key no earlier call used: (wall ms, the comb build's device ms)."""
        w = time.perf_counter()
        be.env_init(tt, nn, b"comb_build_time ck %d" % next(fresh))
        return (time.perf_counter() - w) * 1e3, be.last_comb_build_ms()

    # ---- the builds alone
    shared = {m: [] for m in MODES}
    env_wall = {m: [] for m in MODES}
    keys = {k: {m: [] for m in MODES} for k in key_counts}
    be.set_key_comb(1)
    for rnd in range(args.rounds + 1):  # round 0 warms the buffers and is dropped
        for m in MODES:
            be.set_comb_build(m)
            wall, dev = env_init(n, t)
            assert be.last_comb_build() == m
            if rnd:
                shared[m].append(dev)
                env_wall[m].append(wall)
            for k in key_counts:
                sk, pk = be.member_keys(MASTER, next(fresh), k)
                z = bytes(32 * k)
                be.encrypt_shares(pk, z, z, z, 1, k)
                assert be.last_comb_build() == m and be.last_key_comb() == 1
                if rnd:
                    keys[k][m].append(be.last_comb_build_ms())
    be.set_key_comb(0)
    res["shared_base_build_ms"] = {str(m): spread(shared[m]) for m in MODES}
    res["env_init_wall_ms"] = {str(m): spread(env_wall[m]) for m in MODES}
    res["key_combs_build_ms"] = {str(k): {str(m): spread(keys[k][m]) for m in MODES} for k in key_counts}
    res["key_combs_us_per_key"] = {str(k): {str(m): round(statistics.median(keys[k][m]) * 1e3 / k, 3) for m in MODES}
                                   for k in key_counts}

    def ratio(a, b):
        return round(statistics.median(a) / statistics.median(b), 2)

    res["ratio_mode1_over_mode2"] = {"shared_base": ratio(shared[1], shared[2]),
                                     **{"keys_%d" % k: ratio(keys[k][1], keys[k][2]) for k in key_counts}}

    # ---- what a ceremony under fresh keys pays: env_init + the first ceremony, plaintext and full
    u8 = dict(dtype=torch.uint8, device=torch.device("cuda", 0))
    ta, tb = torch.empty(32 * n * N, **u8), torch.empty(32 * n * N, **u8)
    tr = torch.empty(64 * n * n, **u8)
    be.dealer_coefficients_device(MASTER, 0, 1, 0, n, t, ta.data_ptr(), tb.data_ptr())
    be.enc_randomness_device(MASTER, 0, 1, 0, n, n, t, tr.data_ptr())

    def plain():
        w = time.perf_counter()
        r = be.ceremony_device(ta.data_ptr(), tb.data_ptr(), n, t)
        assert r.n_qualified == n
        return r.ms["total"], (time.perf_counter() - w) * 1e3

    def full(kp):
        w = time.perf_counter()
        r = be.ceremony_full_device(ta.data_ptr(), tb.data_ptr(), tr.data_ptr(), kp[0], kp[1], n, t)
        assert r.n_qualified == n
        return r.ms["total"], (time.perf_counter() - w) * 1e3

    cold = {m: {"env_init_wall": [], "env_init_comb_device": [], "plain_device": [], "plain_wall": [],
                "full_first_device": [], "full_first_wall": [], "full_first_key_combs_device": [],
                "full_warm_device": [], "full_warm_wall": []} for m in MODES}
    for rnd in range(args.rounds + 1):
        for m in MODES:
            be.set_comb_build(m)
            wall, dev = env_init(n, t)
            pd, pw = plain()
            kp = be.member_keys(MASTER, next(fresh), n)
            fd, fw = full(kp)
            kb = be.last_comb_build_ms()
            assert be.last_comb_build() == m
            wd, ww = full(kp)
            if rnd:
                c = cold[m]
                for name, v in (("env_init_wall", wall), ("env_init_comb_device", dev), ("plain_device", pd),
                                ("plain_wall", pw), ("full_first_device", fd), ("full_first_wall", fw),
                                ("full_first_key_combs_device", kb), ("full_warm_device", wd), ("full_warm_wall", ww)):
                    c[name].append(v)
    res["ceremony_n%d_ms" % n] = {str(m): {k: spread(v) for k, v in cold[m].items()} for m in MODES}
    res["cold_start_ms"] = {
        str(m): {"plaintext_env_init_plus_ceremony_wall": round(
                     statistics.median(cold[m]["env_init_wall"]) + statistics.median(cold[m]["plain_wall"]), 3),
                 "full_env_init_plus_first_ceremony_wall": round(
                     statistics.median(cold[m]["env_init_wall"]) + statistics.median(cold[m]["full_first_wall"]), 3)}
        for m in MODES}
    be.set_comb_build(0)
    res["clock_after"] = be.clock_probe()
    be.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
