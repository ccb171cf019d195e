"""One-party, pairs and seats calls on a reduced grid, for comparing two builds of the library point by
point: (64, 31) and (1024, 511), the workloads of receivers_time.py, pairs_time.py, seats_time.py and
seat_chunks_time.py cut down to a few points each (their helpers, their method: synchronous calls, wall
ms, median of 5 after a warm-up, the variants of a point interleaved).

  recv   verify_receivers (round 2) at x = n - 1 and a dense-NAF index: automatic, serial, chunk 8
         commitment_eval at the same two indices in one call
  pairs  commitment_eval_pairs over 1, 64 and 1,024 random (row, index) pairs
  seats  verify_seats (round 2) and commitment_eval_seats at S = 1 and 16: serial walk, chunk 32, automatic
  bfull  (--batch-full) batch_full_time.py's batch at B = 48, n = 64 in chunks of 16 ceremonies, its encryption and
         decryption alone, and one full-mode ceremony at n = 64

--streams 1 runs everything on one stream, where every call also records its phase marks (dkg_ctx_phase_ms).
Prints one JSON line {"library", "device", "clock", "points": {label: {median, min, max, count}}}.  Run it
once per build and round under tools/ab/ab.sh (DKG_AMD_LIB selects the build); profiles/INDEX.md says how
profiles/receivers_refactor_time.json was put together from those lines.
usage: python3 tools/receivers_refactor_time.py [--streams 1] [--batch-full]
"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.receivers_time import committee, indices  # noqa: E402
from tools.seats_time import interleaved, pool_ceremonies  # noqa: E402
from tools.seat_chunks_time import inputs  # noqa: E402

SIZES = ((64, 31), (1024, 511))
SEATS = (1, 16)
PAIRS = (1, 64, 1024)


def size_points(be, n, t, points):
    be.env_init(t, n)
    tag = "n%d" % n
    # one party: the calls of receivers_time.py
    E, _, cols = committee(be, n, t)
    xs = indices(n)[1:]
    for x in xs:
        s, sp = cols[x]

        def recv(chunk):
            def f():
                be.set_receiver_chunk(chunk)
                be.verify_receivers(n, t, 2, [x - 1], E, s, sp)
            return f
        for k, v in interleaved({"auto": recv(0), "serial": recv(t + 1), "L8": recv(8)}).items():
            points["%s recv x%d %s" % (tag, x, k)] = v
    be.set_receiver_chunk(0)
    points["%s recv eval M2" % tag] = interleaved({"e": lambda: be.commitment_eval(n, t, [x - 1 for x in xs], E)})["e"]
    # pairs: pairs_time.py's pairs step
    rng = random.Random(n)
    for count in PAIRS:
        rows = [rng.randrange(n) for _ in range(count)]
        js = [rng.randrange(n) for _ in range(count)]
        points["%s pairs C%d" % (tag, count)] = interleaved({"p": lambda: be.commitment_eval_pairs(n, t, rows, js, E)})["p"]
    # seats: seats_time.py's calls under the routes of seat_chunks_time.py
    pool = max(1, min(max(SEATS), (256 << 20) // (32 * n * n)))
    pooled = pool_ceremonies(be, n, t, pool)
    for S in SEATS:
        Es, cer, js, sc, spc = inputs(be, n, t, S, random.Random(n + S), pooled, pool)
        ref = be.verify_seats(S, n, t, 2, cer, js, Es, sc, spc)

        def seats(mode, chunk, verify):
            def f():
                be.set_seat_eval(mode, chunk)
                if verify:
                    assert be.verify_seats(S, n, t, 2, cer, js, Es, sc, spc) == ref
                else:
                    be.commitment_eval_seats(S, n, t, cer, js, Es)
            return f
        calls = {}
        for mode, chunk, label in ((1, 0, "serial"), (2, min(32, t), "chunked"), (0, 0, "auto")):
            calls["verify " + label] = seats(mode, chunk, True)
            calls["eval " + label] = seats(mode, chunk, False)
        for k, v in interleaved(calls).items():
            points["%s seats S%d %s" % (tag, S, k)] = v
    be.set_seat_eval(0, 0)


def batch_full_points(be, points, B=48, n=64, t=31, chunk=16):
    import torch

    import dkg_amd

    be.env_init(t, n)
    master, dev = b"\xbf" * 32, torch.device("cuda", 0)
    ta = torch.empty(32 * B * n * (t + 1), dtype=torch.uint8, device=dev)
    tb = torch.empty_like(ta)
    tr = torch.empty(64 * B * n * n, dtype=torch.uint8, device=dev)
    be.dealer_coefficients_device(master, 0, B, 0, n, t, ta.data_ptr(), tb.data_ptr())
    be.enc_randomness_device(master, 0, B, 0, n, n, t, tr.data_ptr())
    sk, pk = be.member_keys_batch(master, 0, B, n)
    s = bytes(range(32)) * (B * n * n)  # any scalars: the hybrid stage does not look at them
    r = bytes(tr.cpu().numpy())
    be.set_batch_full_chunk(chunk)
    e1, ct = be.encrypt_shares_batch(pk, s, s, r, B, n)

    def ceremonies():
        res = dkg_amd.ceremony_batch_full_device(be, B, n, t, ta.data_ptr(), tb.data_ptr(), tr.data_ptr(), sk, pk)
        assert res.n_qualified == [n] * B

    calls = {"ceremonies": ceremonies,
             "encrypt": lambda: be.encrypt_shares_batch(pk, s, s, r, B, n),
             "decrypt": lambda: be.decrypt_shares_batch(sk, e1, ct, B, n),
             "single": lambda: be.ceremony_full_device(ta.data_ptr(), tb.data_ptr(), tr.data_ptr(), sk[:32 * n],
                                                       pk[:32 * n], n, t)}
    for k, v in interleaved(calls).items():
        points["n%d bfull B%d %s" % (n, B, k)] = v
    be.set_batch_full_chunk(0)


def main():
    import dkg_amd

    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2, help="dkg_ctx_set_streams (1: the calls record their phases)")
    ap.add_argument("--batch-full", action="store_true", help="add the bfull points")
    args = ap.parse_args()
    be = dkg_amd.Backend(0)
    be.set_streams(args.streams)
    out = {"library": os.path.relpath(dkg_amd._lib.LIB_PATH, ROOT), "streams": args.streams, "device": be.pci_bus_id(),
           "clock": be.clock_probe(), "points": {}}
    for n, t in SIZES:
        size_points(be, n, t, out["points"])
    if args.batch_full:
        batch_full_points(be, out["points"])
    be.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
