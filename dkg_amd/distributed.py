"""Multi-GPU ceremony: one process per GPU, the ceremony sharded by dealer.

Rank r owns dealers [r*n/ws, (r+1)*n/ws) (dkg_shard_range): it generates their commitments and
shares and checks their rows against all n receivers on its GPU (dkg_ceremony_shard_device).  The
protocol's exchange step -- every party learns every complaint (committee.rs:311-331, 370-398) and
the round-3/5 broadcasts (committee.rs:454-467, 790-795) -- is a set of all-gathers (RCCL over xGMI
with the "nccl" backend, gloo in the CPU tests) of:
  * the round-2 / round-4 decision rows, packed as bitmaps (dkg_decisions_pack_device: one ACCEPT
    bit per pair plus a row-kind word -- SELF, MISSING rows and SKIPPED are implied; n=4096: 516
    bytes per row instead of 4096),
  * every dealer's compressed master-key term (A_i0, or g * a_i0 recovered by Lagrange
    interpolation on the owning rank for dealers accused in round 4),
  * each rank's partial final shares (sum over its qualified dealers of s_ij).
The proven runs (run_verify_proven / run_verify_full_proven: each rank verifies the broadcast complaints
against its own dealers, dkg_ceremony_shard_verify_proven_device / _full_proven_device) add to that block
  * one flag word per row (a proven round-1 complaint, a round-4 complaint that holds, no phase-3
    broadcast) and each rank's partial of dissent[j],
still in ONE all-gather, and merge the ranks' verdict arrays with one all_reduce(MAX) per round.
This module holds only the collectives.  The protocol layer runs in the library, behind the C ABI:
dkg_shard_combine_device derives the common outcome (qualified set, complaints, r2 errors, SKIPPED
rows, reconstruction set, r4 errors, Phase4 failure) with the single-GPU drivers' own code, and
dkg_shard_finalise_device the final shares, public shares and mpk (include/dkg_amd.h).
"""
import time
from dataclasses import dataclass
from typing import Any, Dict, Optional

import numpy as np

from .api import shard_range, shard_rows


def dealer_range(rank: int, world_size: int, n: int):
    """Dealers owned by `rank` (dkg_shard_range: contiguous, sizes differ by at most one)."""
    return shard_range(n, world_size, rank)


def max_rows(world_size: int, n: int) -> int:
    """Padded block height R of every rank's gathered rows (dkg_shard_rows)."""
    return shard_rows(n, world_size)


@dataclass
class Decisions:
    dec2: Any                 # [n][n] uint8 tensor on the exchange device
    dec4: Any                 # [n][n] uint8 tensor, SKIPPED rows for disqualified dealers
    qualified: np.ndarray     # [n] uint8
    complaints2: np.ndarray   # [n] int32, complaints raised by receiver j
    r2_error: np.ndarray      # [n] uint8, receiver j saw more than t complaints
    reconstruct: np.ndarray   # [n] uint8, qualified dealers accused in round 4
    r4_error: np.ndarray      # [n] uint8, receiver j saw fewer than t+1 honest dealers in round 4
    phase4_error: bool        # qualified minus reconstructable <= t: Phase4::proceed fails (:673-677)


class ShardResult:
    """One rank's outputs of a sharded ceremony.
    final_share  [n][32] s_j (committee.rs:454-462) and public_share [n][32] g * s_j (:463-467): bytes,
                 copied from the device when first read (a device copy is kept, so a later run does
                 not change them; a timed loop that never reads them pays no host round trip)
    mpk          32 bytes (committee.rs:790-795); None when Phase4 fails
    ms_shard     device time of this rank's share gen + checks
    ms_steps     host wall ms of the steps after the shard: "exchange" (the all-gather, fenced),
                 "combine" (dkg_shard_combine_device + outcome copies), "recon" (round-4
                 reconstruction + its gather; 0 when nobody was accused), "finalise"
                 (dkg_shard_finalise_device)"""

    def __init__(self, decisions: Decisions, final_share, public_share, mpk: Optional[bytes], ms_shard: float,
                 ms_steps: Optional[Dict[str, float]] = None, verdict=None, verdict4=None, dissent=None,
                 finalise_status: Optional[int] = None, recovery_index: Optional[int] = None):
        self.decisions, self._fs, self._pub = decisions, final_share, public_share
        self.mpk, self.ms_shard, self.ms_steps = mpk, ms_shard, dict(ms_steps or {})
        # the proven runs (run_verify_proven / run_verify_full_proven), else None: the ceremony's merged
        # verdict lists (round 2: full mode only), dissent [n] (full mode), and the finalising parties'
        # common outcome in the dkg_amd._lib.FIN_* codes with the dealer of INSUFFICIENT / PANIC
        self.verdict, self.verdict4, self.dissent = verdict, verdict4, dissent
        self.finalise_status, self.recovery_index = finalise_status, recovery_index

    @staticmethod
    def _host(v):
        return v if v is None or isinstance(v, (bytes, bytearray)) else bytes(v.cpu().numpy())

    @property
    def final_share(self) -> Optional[bytes]:
        self._fs = self._host(self._fs)
        return self._fs

    @property
    def public_share(self) -> Optional[bytes]:
        self._pub = self._host(self._pub)
        return self._pub


class ShardedCeremony:
    """One rank's view of a dealer-sharded ceremony.  `be` is this rank's dkg_amd.Backend (its GPU),
    `dist` an initialised torch.distributed, `device` the torch device the exchanged buffers live on
    (cuda:local for RCCL; cpu works with gloo)."""

    def __init__(self, be, dist, n: int, t: int, device, packed: bool = True):
        import torch

        self.torch = torch
        self.be, self.dist, self.n, self.t, self.dev = be, dist, n, t, device
        self.packed = packed
        self.ws, self.rank = dist.get_world_size(), dist.get_rank()
        self.staged = dist.get_backend() == "gloo" and getattr(device, "type", str(device)) != "cpu"
        self.d0, self.d1 = dealer_range(self.rank, self.ws, n)
        D, R = self.d1 - self.d0, max_rows(self.ws, n)
        u8 = dict(dtype=torch.uint8, device=device)
        # One send block per rank, gathered in ONE collective: [round-2 rows | round-4 rows | master-key
        # terms [R][32] | partial final shares [n][32]], the rows packed ([R][W+1] u32 bitmaps,
        # dkg_packed_row_words) or raw ([R][n] bytes).  The library writes straight into its views.
        if packed:
            from .api import packed_row_words

            self.W1 = packed_row_words(n)
            S2 = 4 * R * self.W1
        else:
            S2 = R * n
        self.S2, self.S = S2, 2 * S2 + R * 32 + n * 32
        self.send = torch.zeros(self.S, **u8)
        self.A0 = self.send[2 * S2:2 * S2 + R * 32]
        self.part = self.send[2 * S2 + R * 32:]
        if packed:
            self.dec2 = torch.zeros(R * n, **u8)  # raw rows, packed into the send block
            self.dec4 = torch.zeros(R * n, **u8)
            self.p2 = self.send[:S2].view(torch.int32)
            self.p4 = self.send[S2:2 * S2].view(torch.int32)
            i32 = dict(dtype=torch.int32, device=device)
            self.g_dec2 = torch.empty(self.ws * R * self.W1, **i32)
            self.g_dec4 = torch.empty(self.ws * R * self.W1, **i32)
        else:
            self.dec2, self.dec4 = self.send[:S2], self.send[S2:2 * S2]
            self.p2 = self.p4 = None  # the library writes the raw rows straight into the block
            self.g_dec2 = torch.empty(self.ws * R * n, **u8)
            self.g_dec4 = torch.empty(self.ws * R * n, **u8)
        self.g_all = torch.empty(self.ws * self.S, **u8)
        self.g_A0 = torch.empty(self.ws * R * 32, **u8)
        self.g_part = torch.empty(self.ws * n * 32, **u8)
        self.c_dec2 = torch.empty(n * n, **u8)   # compacted by the combine
        self.c_dec4 = torch.empty(n * n, **u8)
        self.fs = torch.empty(n * 32, **u8)
        self.pub = torch.empty(n * 32, **u8)
        self.D, self.R = D, R
        self.p_send = None          # the proven runs' send block (_proven_init), allocated on first use
        self._last_proven = False

    def _fence(self):
        """The library runs on its own HIP streams: before it reads buffers torch produced (the
        gathered rows, uploads) or overwrites buffers a collective may still read, the work queued
        on torch's stream -- including an RCCL collective, which torch's current stream waits for --
        must have completed."""
        if getattr(self.dev, "type", str(self.dev)) == "cuda":
            self.torch.cuda.current_stream(self.dev).synchronize()

    def _all_gather(self, out, inp):
        if self.staged:  # gloo with device buffers: through host memory (rehearsal / CPU runs)
            o = out.cpu()
            self.dist.all_gather_into_tensor(o, inp.cpu())
            out.copy_(o)
        else:
            self.dist.all_gather_into_tensor(out, inp)

    def _pack(self, dec, out):
        """This rank's raw rows [D][n] -> its packed block [R][W+1] (dkg_decisions_pack_device)."""
        self.be.decisions_pack_device(self.R, self.D, self.n, self.d0, dec.data_ptr(), out.data_ptr())

    def exchange_bytes(self, proven: Optional[bool] = None) -> int:
        """Bytes one rank contributes to the all-gather of one ceremony (without the round-4
        reconstruction's second gather of the master-key terms).  proven: the send block of the proven
        runs, which carries [R] flag words and [n] dissent words more; None = the kind of the last run."""
        if proven is None:
            proven = self._last_proven
        return self.S + 4 * self.R + 4 * self.n if proven else self.S

    # ---- the proven runs: each rank verifies the complaints against its own dealers
    def _proven_init(self):
        """The proven runs' send block, still gathered in ONE collective: the packed block's [round-2
        rows | round-4 rows | master-key terms | partial final shares], then [R] u32 flag words and [n]
        i32 dissent partials.  The existing runs' block and buffers stay as they are."""
        if not self.packed:
            raise ValueError("the proven runs exchange packed rows: ShardedCeremony(packed=True)")
        if self.p_send is not None:
            return
        torch, R, n, ws, S2 = self.torch, self.R, self.n, self.ws, self.S2
        u8 = dict(dtype=torch.uint8, device=self.dev)
        i32 = dict(dtype=torch.int32, device=self.dev)
        self.SP = self.S + 4 * R + 4 * n
        self.p_send = torch.zeros(self.SP, **u8)
        self.pp2 = self.p_send[:S2].view(torch.int32)
        self.pp4 = self.p_send[S2:2 * S2].view(torch.int32)
        self.pA0 = self.p_send[2 * S2:2 * S2 + R * 32]
        self.ppart = self.p_send[2 * S2 + R * 32:self.S]
        self.pflags = self.p_send[self.S:self.S + 4 * R].view(torch.int32)
        self.pdis = self.p_send[self.S + 4 * R:].view(torch.int32)
        self.g_allp = torch.empty(ws * self.SP, **u8)
        self.g_flags = torch.empty(ws * R, **i32)
        self.g_dis = torch.empty(ws * n, **i32)

    def _merge_verdicts(self, v):
        """One all_reduce(MAX) over the ranks' verdict arrays: COMPLAINT_NOT_OWNED is below every real code
        and exactly one rank owns each complaint.  Staged through the host under gloo, as _all_gather."""
        if not len(v):
            return []
        host = self.dist.get_backend() == "gloo"
        tt = self.torch.tensor(list(v), dtype=self.torch.int32, device="cpu" if host else self.dev)
        self.dist.all_reduce(tt, op=self.dist.ReduceOp.MAX)
        return tt.cpu().tolist()

    def run_verify_proven(self, d_E: int, d_A: int, d_s: int, d_sp: int, accusers4, accused4, share4: bytes,
                          randomness4: bytes, fetched1: Optional[bytes] = None, fetched3: Optional[bytes] = None,
                          finalise: bool = True) -> ShardResult:
        """run_verify whose reconstructable set follows the PROVEN round-4 complaints (round 2 keeps the
        rejection rule: plaintext shares).  The whole broadcast complaint list goes to every rank (1-based
        indices; share4 / randomness4 [C4][32]); fetched1 / fetched3: this rank's rows' intake masks."""
        self._proven_init()
        self._fence()
        ms, v4 = self.be.ceremony_shard_verify_proven_device(
            self.n, self.t, self.d0, self.d1, d_E, d_A, d_s, d_sp, accusers4, accused4, share4, randomness4,
            self.dec2.data_ptr(), self.dec4.data_ptr(), self.pA0.data_ptr(), self.ppart.data_ptr(), self.R,
            self.pflags.data_ptr(), fetched1=fetched1, fetched3=fetched3)
        return self._finish(ms, finalise, d_s, proven=(False, [], v4))

    def run_verify_full_proven(self, d_E: int, d_A: int, d_e1: int, d_ct: int, sk: bytes, pk: bytes, accusers,
                               accused, proofs: bytes, accusers4, accused4, share4: bytes, randomness4: bytes,
                               fetched1: Optional[bytes] = None, fetched3: Optional[bytes] = None,
                               finalise: bool = True) -> ShardResult:
        """run_verify_full with both sets decided by the proven complaints: round-1 complaints (accusers,
        accused, proofs [C][192]) against this ceremony's own ciphertexts, round-4 complaints as
        run_verify_proven."""
        self._proven_init()
        self._fence()
        ms, v, v4 = self.be.ceremony_shard_verify_full_proven_device(
            self.n, self.t, self.d0, self.d1, d_E, d_A, d_e1, d_ct, sk, pk, accusers, accused, proofs, accusers4,
            accused4, share4, randomness4, self.dec2.data_ptr(), self.dec4.data_ptr(), self.pA0.data_ptr(),
            self.ppart.data_ptr(), self.R, self.pflags.data_ptr(), self.pdis.data_ptr(), fetched1=fetched1,
            fetched3=fetched3)
        return self._finish(ms, finalise, None, proven=(True, v, v4))

    def _exchange(self, send, g_all, p2, p4, tail=()):
        """All-gather every rank's send block (one collective), then split the gathered [ws][len(send)]
        blocks on the device into g_dec2, g_dec4, g_A0, g_part and `tail`'s (tensor, bytes per rank)."""
        if self.packed:
            self._pack(self.dec2, p2)
            self._pack(self.dec4, p4)
        self._all_gather(g_all, send)
        ws, u8 = self.ws, self.torch.uint8
        g = g_all.view(ws, -1)
        parts = [(self.g_dec2, self.S2), (self.g_dec4, self.S2), (self.g_A0, self.R * 32), (self.g_part, self.n * 32)]
        at = 0
        for dst, size in parts + list(tail):
            dst.view(u8).view(ws, size).copy_(g[:, at:at + size])
            at += size
        return tuple(dst for dst, _ in parts + list(tail))

    def exchange(self):
        """The exchange of the send block: the decision rows (round 2, round 4; packed bitmaps
        [ws][R][W+1] or bytes [ws][R][n]), the master-key terms [ws][R][32] and the partial final shares
        [ws][n][32]."""
        return self._exchange(self.send, self.g_all, self.p2, self.p4)

    def exchange_proven(self):
        """exchange() for the proven runs' block: also the gathered flag words [ws][R] and dissent
        partials [ws][n]."""
        return self._exchange(self.p_send, self.g_allp, self.pp2, self.pp4,
                              ((self.g_flags, 4 * self.R), (self.g_dis, 4 * self.n)))

    def run(self, d_a: int, d_b: int, finalise: bool = True) -> ShardResult:
        """Share gen + rounds 2/4 for this rank's dealers (device pointers d_a, d_b to its [D][t+1][32]
        coefficients), exchange, combine.  With finalise, also the round-3 final shares and public
        shares and the master public key, on the GPU."""
        self._fence()
        ms = self.be.ceremony_shard_device(self.n, self.t, self.d0, self.d1, d_a, d_b, self.dec2.data_ptr(),
                                           self.dec4.data_ptr(), self.A0.data_ptr(), self.part.data_ptr())
        return self._finish(ms, finalise)

    def run_verify(self, d_E: int, d_A: int, d_s: int, d_sp: int, finalise: bool = True) -> ShardResult:
        """Rounds 2-5 on received broadcasts: this rank's dealers' commitments d_E, d_A [D][t+1][32]
        (compressed, as broadcast in phases 1 and 3) and their shares d_s, d_sp [D][n][32]."""
        self._fence()
        ms = self.be.ceremony_shard_verify_device(self.n, self.t, self.d0, self.d1, d_E, d_A, d_s, d_sp,
                                                  self.dec2.data_ptr(), self.dec4.data_ptr(),
                                                  self.A0.data_ptr(), self.part.data_ptr())
        return self._finish(ms, finalise, d_s)

    def run_full(self, d_a: int, d_b: int, d_r: int, sk: bytes, pk: bytes, finalise: bool = True,
                 d_e1: Optional[int] = None, d_ct: Optional[int] = None) -> ShardResult:
        """run in full (encrypted-share) mode: this rank's dealers' shares are hybrid-encrypted to the n
        sorted member keys (d_r: device [D][n][2][32] randomness; sk, pk: [n][32] bytes), decrypted by
        all n receivers and checked (dkg_ceremony_shard_full_device).  d_e1 / d_ct optionally receive
        the rank's round-1 ciphertexts.  The reconstruction reads the remembered decrypted shares."""
        self._fence()
        ms = self.be.ceremony_shard_full_device(self.n, self.t, self.d0, self.d1, d_a, d_b, d_r, sk, pk,
                                                self.dec2.data_ptr(), self.dec4.data_ptr(), self.A0.data_ptr(),
                                                self.part.data_ptr(), d_e1, d_ct)
        return self._finish(ms, finalise, None)

    def run_verify_full(self, d_E: int, d_A: int, d_e1: int, d_ct: int, sk: bytes,
                        finalise: bool = True) -> ShardResult:
        """run_verify on received ciphertexts: d_e1, d_ct device [D][n][2][32] of this rank's dealers."""
        self._fence()
        ms = self.be.ceremony_shard_verify_full_device(self.n, self.t, self.d0, self.d1, d_E, d_A, d_e1, d_ct, sk,
                                                       self.dec2.data_ptr(), self.dec4.data_ptr(),
                                                       self.A0.data_ptr(), self.part.data_ptr())
        return self._finish(ms, finalise, None)

    def _finish(self, ms: float, finalise: bool, d_s: Optional[int] = None, proven=None) -> ShardResult:
        """The steps after the shard call.  proven: a proven run's (full, verdict, verdict4) -- this rank's
        verdict arrays -- whose block also carries the flag words and dissent partials."""
        from ._lib import FIN_PANIC, FIN_PHASE4_ERROR

        n, t, ws = self.n, self.t, self.ws
        self._last_proven = proven is not None
        A0 = self.A0 if proven is None else self.pA0  # this rank's terms in the block that was sent
        steps, extra = {}, {}
        c0 = time.perf_counter()
        if proven is None:
            self.exchange()
        else:
            full, v, v4 = proven
            self.exchange_proven()
            verdict, verdict4 = self._merge_verdicts(v), self._merge_verdicts(v4)
        self._fence()
        c1 = time.perf_counter()
        steps["exchange"] = (c1 - c0) * 1e3
        if proven is None:
            o = self.be.shard_combine_device(n, t, ws, self.g_dec2.data_ptr(), self.g_dec4.data_ptr(),
                                             self.c_dec2.data_ptr(), self.c_dec4.data_ptr(), packed=self.packed,
                                             arrays=True)
            no_mpk = o.phase4_error
        else:
            o, dissent, status, index = self.be.shard_combine_proven_device(
                n, t, ws, self.g_dec2.data_ptr(), self.g_dec4.data_ptr(), self.g_flags.data_ptr(),
                self.g_dis.data_ptr() if full else None, full, self.c_dec2.data_ptr(), self.c_dec4.data_ptr())
            extra = dict(verdict=verdict if full else None, verdict4=verdict4, dissent=dissent,
                         finalise_status=status, recovery_index=index)
            # nobody finalises after a Phase4 failure, and a panic of every party's finalise leaves no mpk
            no_mpk = status in (FIN_PHASE4_ERROR, FIN_PANIC)
        dec = Decisions(self.c_dec2.view(n, n), self.c_dec4.view(n, n), np.array(o.qualified, dtype=np.uint8),
                        np.array(o.complaints2, dtype=np.int32), np.array(o.r2_error, dtype=np.uint8),
                        np.array(o.reconstruct, dtype=np.uint8), np.array(o.r4_error, dtype=np.uint8),
                        o.phase4_error)
        c2 = time.perf_counter()
        steps["combine"] = (c2 - c1) * 1e3
        if not finalise:
            return ShardResult(dec, None, None, None, ms, steps, **extra)
        if dec.reconstruct.any() and not no_mpk:
            # a dealer accused in round 4 (committee.rs:660-670) enters mpk as g * a_i0 over the
            # disclosing final parties' shares (:747-789): the owning rank replaces its term and the
            # terms are gathered again (the interpolation points depend on every rank's rows).  Fewer
            # than t disclosing parties: nobody recovers (:779-781), the same verdict on every rank.
            no_mpk = self.be.ceremony_shard_recon_device(n, t, self.d0, self.d1, dec.qualified, dec.reconstruct, d_s,
                                                         A0.data_ptr(), dec.r2_error, dec.r4_error)
            if not no_mpk:
                self._all_gather(self.g_A0, A0)
                self._fence()
        c3 = time.perf_counter()
        steps["recon"] = (c3 - c2) * 1e3
        mpk = self.be.shard_finalise_device(n, t, ws, self.g_A0.data_ptr(), self.g_part.data_ptr(), dec.qualified,
                                            no_mpk, self.fs.data_ptr(), self.pub.data_ptr())
        # device copies of this run's shares (the buffers are reused), read back only when asked for
        fs, pub = self.fs.clone(), self.pub.clone()
        steps["finalise"] = (time.perf_counter() - c3) * 1e3
        return ShardResult(dec, fs, pub, None if no_mpk else mpk, ms, steps, **extra)
