"""Python host API over the C ABI, mirroring the reference's operator surface for this path.

Reference interface -> here:
  Environment::init(threshold, nr_members, ck_gen_bytes)      committee.rs:72-83  -> Environment
  PrimeGroupElement::vartime_multiscalar_multiplication        traits.rs:234-237   -> Backend.msm_batch
  Mul<Scalar> (generator / h)                                  traits.rs:212       -> Backend.fixed_base_batch
  Polynomial::evaluate                                         polynomial.rs:68-74 -> Backend.poly_eval_batch
  PrimeGroupElement::from_bytes (validity)                     groups.rs:78-81     -> Backend.points_valid
  Phases<Initialise>::init (all dealers)                       committee.rs:124-216 -> Backend.share_gen
  Phases<Phase1>::proceed / Phases<Phase3>::proceed checks     committee.rs:273-338, 520-559
                                                               -> Backend.verify_pairs / verify_receiver
  the all-parties test driver (full_valid_run)                 committee.rs:1518-1656 -> Backend.ceremony
Scalars and points are 32-byte encodings (bytes), exactly the reference's wire values.
"""
import ctypes
from collections.abc import Sequence
from dataclasses import dataclass
from typing import List, Optional

from . import _lib
from ._lib import BatchOut, CeremonyOut, DkgError

CK_DEFAULT = b"Example of a shared string."


def _check(ctx, rc):
    if rc != _lib.DKG_OK:
        msg = _lib.lib().dkg_ctx_last_error(ctx).decode() if ctx else ""
        raise DkgError(rc, msg)


def env_check(threshold: int, nr_members: int) -> None:
    """committee.rs:73 `assert!(threshold < (nr_members + 1) / 2)` -> DkgError(DKG_E_ARG)."""
    rc = _lib.lib().dkg_env_check(threshold, nr_members)
    if rc != _lib.DKG_OK:
        raise DkgError(rc, f"threshold {threshold} must be < (nr_members + 1) / 2 = {(nr_members + 1) // 2}")


def dealer_coefficients(master: bytes, ceremony: int, d0: int, D: int, t: int):
    """Seeded Polynomial::random pair per dealer (hiding first, committee.rs:143-146): (a, b)."""
    N = t + 1
    a = ctypes.create_string_buffer(32 * D * N)
    b = ctypes.create_string_buffer(32 * D * N)
    rc = _lib.lib().dkg_dealer_coeffs(master, ceremony, d0, D, t, a, b)
    if rc != _lib.DKG_OK:
        raise DkgError(rc, "dealer_coeffs")
    return a.raw, b.raw


def enc_randomness(master: bytes, ceremony: int, d0: int, D: int, n: int, t: int) -> bytes:
    """Encryption randomness [D][n][2][32] continuing each dealer's seeded stream (committee.rs:171-172)."""
    r = ctypes.create_string_buffer(max(64 * D * n, 1))
    rc = _lib.lib().dkg_enc_randomness(master, ceremony, d0, D, n, t, r)
    if rc != _lib.DKG_OK:
        raise DkgError(rc, "enc_randomness")
    return r.raw[:64 * D * n]


def split_multipliers(n: int, L: int, pieces: int):
    """Short recombination vectors [(b_j, a_j1, ..)] of receivers j = 1..n for a `pieces`-way split
    of piece length L (a_ju = b_j j^(uL) mod l; dkg_split_multipliers, host-only)."""
    mag = ctypes.create_string_buffer(32 * n * pieces)
    sign = ctypes.create_string_buffer(n * pieces)
    rc = _lib.lib().dkg_split_multipliers(n, L, pieces, mag, sign)
    if rc != _lib.DKG_OK:
        raise DkgError(rc, "split_multipliers")
    sg = [1 if b < 128 else -1 for b in sign.raw]
    m = mag.raw  # one copy (each .raw access copies the whole buffer)
    return [[sg[j * pieces + u] * int.from_bytes(m[(j * pieces + u) * 32:(j * pieces + u + 1) * 32], "little")
             for u in range(pieces)] for j in range(n)]


def _carray(ctype, count: int, values=()):
    """A ctypes array of `count` entries (at least one, so that it is never a null pointer)."""
    return (ctype * max(count, 1))(*values)


@dataclass
class CeremonyResult:
    n: int
    t: int
    mpk: bytes
    qualified: List[int]
    r2_error: List[int]
    r4_error: List[int]
    complaints2: List[int]
    reconstruct: List[int]
    n_qualified: int
    phase4_error: int
    ms: dict
    E: Optional[bytes] = None
    A: Optional[bytes] = None
    s: Optional[bytes] = None
    s_prime: Optional[bytes] = None
    dec2: Optional[bytes] = None
    dec4: Optional[bytes] = None
    final_share: Optional[bytes] = None
    public_share: Optional[bytes] = None


@dataclass
class ProvenResult:
    """A ceremony whose reconstructable set follows the proven round-4 complaints
    (Phases<Phase4>::proceed, committee.rs:625-688).  verdict4[c]: 0 valid, 2 / 3 false claims, -1 the E
    row does not decode, COMPLAINT_IGNORED (accused disqualified), COMPLAINT_NO_PHASE3 (valid
    unverified).  finalise_status: dkg_amd._lib.FIN_*, the finalising parties' common outcome;
    recovery_index the 0-based dealer of FIN_INSUFFICIENT / FIN_PANIC, else -1.  Full mode adds the
    round-1 complaints' verdict and dissent (ceremony_verify_full_complaints)."""
    result: CeremonyResult
    verdict4: List[int]
    finalise_status: int
    recovery_index: int
    verdict: Optional[List[int]] = None
    dissent: Optional[List[int]] = None


@dataclass
class PartyFinalise:
    """Per-party outcome of Phases<Phase5>::finalise (dkg_finalise_parties): status[p] is one of
    dkg_amd._lib.FIN_* and recovery_index[p] the dealer of InsufficientSharesForRecovery (else -1)."""
    mpk: List[bytes]
    status: List[int]
    recovery_index: List[int]


@dataclass
class PublicShares:
    """dkg_public_shares: V [B][M][32] (32 zero bytes unless status is DKG_PS_OK), status and which per
    (ceremony, index) as dkg_public_share_status gives them, S [B][t+1][32] the summed commitments or None."""
    V: bytes
    status: List[int]
    which: List[int]
    S: Optional[bytes]


class Backend:
    """One GPU (one process per GPU).  Owns a dkg_ctx."""

    def __init__(self, device: int = 0):
        L = _lib.lib()
        h = ctypes.c_void_p()
        rc = L.dkg_ctx_create(device, ctypes.byref(h))
        if rc != _lib.DKG_OK:
            raise DkgError(rc, f"dkg_ctx_create(device={device}) failed (is a gfx950 GPU visible?)")
        self._ctx = h
        self.device = device
        self.h: Optional[bytes] = None

    def close(self):
        if self._ctx:
            _lib.lib().dkg_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def ctx(self):
        return self._ctx

    def set_streams(self, nsub: int):
        """Dealer-chunk streams of the round-2/4 checks (1 = serialised, phase times recorded)."""
        _check(self._ctx, _lib.lib().dkg_ctx_set_streams(self._ctx, nsub))

    def set_verify_mode(self, mode):
        """0 / "group": difference tables (every P_i(j) in the group, default); 1 / "interp":
        committee verification by interpolation (identical decisions; dkg_ctx_set_verify_mode)."""
        m = {"group": 0, "interp": 1}.get(mode, mode)
        _check(self._ctx, _lib.lib().dkg_ctx_set_verify_mode(self._ctx, int(m)))

    def fallback_rows(self) -> int:
        return _lib.lib().dkg_ctx_fallback_rows(self._ctx)

    def set_split(self, pieces: int):
        """Degree split of the difference tables (0 = cost model, 1 = off); results are identical."""
        _check(self._ctx, _lib.lib().dkg_ctx_set_split(self._ctx, pieces))

    def set_field_mode(self, mode: int):
        """Field multiplication of the verification kernels: 0 by occupancy, 1 product scanning,
        2 column sums; results are identical."""
        _check(self._ctx, _lib.lib().dkg_ctx_set_field_mode(self._ctx, mode))

    def set_binomial(self, mode: int):
        """Binomial schedule (dkg_ctx_set_binomial): 0 (default) per-wave Horner loops for tables of
        many column groups, else one launch per step with lane pairs for the latency-bound steps; 1
        per step without lane pairs; 2 per step with lane pairs everywhere; 3 per step as 0; 4 per
        wave always; 5 per wave always with each item's operand prefetched during the previous item."""
        _check(self._ctx, _lib.lib().dkg_ctx_set_binomial(self._ctx, mode))

    def set_check(self, mode: int):
        """Fused round-2/4 checks: 0 one launch over both combs (default), 1 one launch per comb with
        g*s parked between them (dkg_ctx_set_check); decisions are identical."""
        _check(self._ctx, _lib.lib().dkg_ctx_set_check(self._ctx, mode))

    def set_stepping(self, mode: int):
        """Stepping slots: 0 cost model, 1 one per column (all pieces of a split table), 2 one per
        piece, 3 as 0 without the dead-position repack of short unsplit tables; results are identical."""
        _check(self._ctx, _lib.lib().dkg_ctx_set_stepping(self._ctx, mode))

    def set_combine(self, mode: int):
        """Recombination of a degree split: 0 short lattice multipliers for 2..4 pieces (default),
        1 powers of y = j^L; 3 short multipliers as per-scalar NAF chains at every U (0 and 2 run
        pairwise joint-sparse-form chains at U = 2, 4); decisions are identical (dkg_ctx_set_combine)."""
        _check(self._ctx, _lib.lib().dkg_ctx_set_combine(self._ctx, mode))

    def set_stepping_formula(self, mode: int):
        """Stepping additions: 0 dedicated formula with complete redo of the workgroups that met an
        exceptional pair (default), 1 complete formula only; decisions are identical."""
        _check(self._ctx, _lib.lib().dkg_ctx_set_stepping_formula(self._ctx, mode))

    def stepping_redos(self) -> int:
        """Workgroups of the last verification's stepping redone by the complete formula."""
        r = _lib.lib().dkg_ctx_stepping_redos(self._ctx)
        if r < 0:
            raise DkgError(_lib.DKG_E_DEVICE, "dkg_ctx_stepping_redos failed")
        return r

    def zero_tests(self, limbs) -> list:
        """Test aid (dkg_zero_tests): for each element of ten 32-bit limbs, the tuple (one-limb filter,
        full zero test, filtered guard) as the device computes them."""
        count = len(limbs)
        arr = (ctypes.c_uint32 * (10 * max(count, 1)))(*[v for el in limbs for v in el])
        out = ctypes.create_string_buffer(3 * max(count, 1))
        _check(self._ctx, _lib.lib().dkg_zero_tests(self._ctx, count, arr, out))
        return [tuple(out.raw[3 * i:3 * i + 3]) for i in range(count)]

    # words per operand tuple (in, out) of dkg_fe_ops / dkg_sc_ops, by op (include/dkg_amd.h)
    FE_OPS = {"mul": (0, 20, 10), "sq": (1, 10, 10), "mul2": (2, 40, 20), "sq2": (3, 20, 20),
              "mul_small": (4, 11, 10), "carry": (5, 10, 10), "add": (6, 20, 10), "sub": (7, 20, 10),
              "neg": (8, 10, 10), "dbl": (9, 10, 10), "invert": (10, 10, 10), "pow22523": (11, 10, 10),
              "tobytes": (12, 10, 10), "frombytes": (13, 8, 10), "abs": (14, 10, 10)}
    SC_OPS = {"reduce9": (0, 9, 8), "reduce256": (1, 8, 8), "reduce512": (2, 16, 8), "add": (3, 16, 8),
              "sub": (4, 16, 8), "neg": (5, 8, 8), "mul_small_add": (6, 17, 8), "horner2": (7, 25, 8),
              "lazy": (8, 20, 18), "mont_mul": (9, 16, 8), "mul": (10, 16, 8), "mont_inv": (11, 8, 8),
              "radix16": (12, 8, 16)}

    @staticmethod
    def _word_ops(table, op, tuples):
        code, win, wout = table[op]
        count = len(tuples)
        flat = [w for tup in tuples for w in tup]
        if len(flat) != win * count:
            raise ValueError(f"{op}: every operand tuple takes {win} words")
        arr = (ctypes.c_uint32 * max(len(flat), 1))(*flat)
        out = (ctypes.c_uint32 * max(wout * count, 1))()
        return code, count, wout, arr, out

    def fe_ops(self, flavour: int, op: str, tuples) -> list:
        """Test aid (dkg_fe_ops): the field primitive `op` (a key of FE_OPS) on each tuple of raw 32-bit
        limb words, in flavour 1 (product scanning) or 2 (column sums); one list of output words per tuple."""
        code, count, wout, arr, out = self._word_ops(self.FE_OPS, op, tuples)
        _check(self._ctx, _lib.lib().dkg_fe_ops(self._ctx, flavour, code, count, arr, out))
        return [list(out[wout * i:wout * (i + 1)]) for i in range(count)]

    def sc_ops(self, op: str, tuples) -> list:
        """Test aid (dkg_sc_ops): the scalar primitive `op` (a key of SC_OPS) on each tuple of 32-bit
        words; one list of output words per tuple."""
        code, count, wout, arr, out = self._word_ops(self.SC_OPS, op, tuples)
        _check(self._ctx, _lib.lib().dkg_sc_ops(self._ctx, code, count, arr, out))
        return [list(out[wout * i:wout * (i + 1)]) for i in range(count)]

    def binomial_reruns(self) -> int:
        """1 when the last ceremony / shard call reran its verification with the complete formula
        (a dedicated addition of the per-step binomial met an exceptional pair), else 0."""
        return _lib.lib().dkg_ctx_binomial_reruns(self._ctx)

    def binomial_wave_redos(self) -> int:
        """Test aid: (piece, 64-column group) flag words of the per-wave binomial that the last
        verification marked and rebuilt with the complete formula (0 when the complete formula ran)."""
        r = _lib.lib().dkg_ctx_binomial_wave_redos(self._ctx)
        if r < 0:
            raise DkgError(_lib.DKG_E_DEVICE, "dkg_ctx_binomial_wave_redos failed")
        return r

    def clock_probe(self, iters: int = 200_000) -> dict:
        """Shader clock under full VALU occupancy (dkg_ctx_clock_probe): {"sclk_mhz", "busy_ms"}."""
        mhz, ms = ctypes.c_double(), ctypes.c_double()
        _check(self._ctx, _lib.lib().dkg_ctx_clock_probe(self._ctx, iters, ctypes.byref(mhz), ctypes.byref(ms)))
        return {"sclk_mhz": mhz.value, "busy_ms": ms.value}

    def pci_bus_id(self) -> str:
        """PCI bus id of this context's device ("dddd:bb:dd.f")."""
        return device_pci_bus_id(self.device)

    def set_addends(self, mode: int):
        """Addends of the short-multiplier recombination: 0 affine Niels (default), 1 cached
        projective; decisions are identical (dkg_ctx_set_addends)."""
        _check(self._ctx, _lib.lib().dkg_ctx_set_addends(self._ctx, mode))

    def last_combine(self) -> int:
        """0 no split, 1 powers of y, 2 short multipliers (the last verification)."""
        return _lib.lib().dkg_ctx_last_combine(self._ctx)

    def last_binomial(self) -> int:
        """0 one launch per Horner step, 1 per-wave loops (k_binom_wave) in the last verification."""
        return _lib.lib().dkg_ctx_last_binomial(self._ctx)

    def last_split(self) -> int:
        return _lib.lib().dkg_ctx_last_split(self._ctx)

    def last_split_len(self) -> int:
        """Piece length L of the last split (the last piece holds t + 1 - (U - 1) L coefficients)."""
        return _lib.lib().dkg_ctx_last_split_len(self._ctx)

    def set_overlap(self, on: bool):
        """Verify rounds 2 and 4 as one fused pipeline (default) or in protocol order."""
        _check(self._ctx, _lib.lib().dkg_ctx_set_overlap(self._ctx, 1 if on else 0))

    def phase_times(self, tag="r24") -> dict:
        """Device ms of binomial / stepping / combine / check in the last ceremony's checks: tag "r24" (rounds
        2 and 4 fused, the default schedule), "r2" or "r4" (protocol order), "full" (the hybrid
        encryption / decryption kernels of the last full-mode ceremony), "recv" (the last one-party call:
        commitment_eval, verify_receivers, party_round2), "pairs" (the last commitment_eval_pairs), "pubshares" (the last commitment_sum / public_shares), "seats" (the last
        commitment_eval_seats, verify_seats, party_round2_seats; lagrange / mpk: the last finalise_seats; commit /
        deal_*: the last party_round1_seats).  Only recorded with set_streams(1); -1 otherwise."""
        L = _lib.lib()
        if isinstance(tag, int):
            tag = f"r{tag}"
        names = (("interpolate", "coef_check", "decide", "fallback") if tag == "interp"
                 else ("decrypt", "decode", "chunks", "fold", "check", "prove") if tag == "recv"
                 else ("decode", "eval") if tag == "pairs"
                 else ("decode", "sum", "eval", "disclosed") if tag == "pubshares"
                 else ("decrypt", "decode", "eval", "fold", "check", "prove", "lagrange", "mpk", "commit", "deal_e1", "deal_mul",
                       "deal_encode", "deal_sym") if tag == "seats"
                 else ("enc_mul", "enc_encode", "enc_sym", "dec_decode", "dec_mul", "dec_encode", "dec_sym")
                 if tag == "full" else ("binomial", "stepping", "combine", "check"))
        return {k: L.dkg_ctx_phase_ms(self._ctx, f"{tag}.{k}".encode()) for k in names}

    def env_init(self, threshold: int, nr_members: int, ck_gen_bytes: bytes = CK_DEFAULT) -> bytes:
        out = ctypes.create_string_buffer(32)
        _check(self._ctx, _lib.lib().dkg_env_init(self._ctx, threshold, nr_members, ck_gen_bytes,
                                                   len(ck_gen_bytes), out))
        self.h = out.raw
        return out.raw

    # ---- trait-level batches
    def msm_batch(self, scalars: bytes, points: bytes, B: int, N: int) -> bytes:
        out = ctypes.create_string_buffer(32 * max(B, 1))
        _check(self._ctx, _lib.lib().dkg_msm_batch(self._ctx, B, N, scalars, points, out))
        return out.raw[: 32 * B]

    def fixed_base_batch(self, scalars: bytes, base: Optional[bytes] = None) -> bytes:
        count = len(scalars) // 32
        out = ctypes.create_string_buffer(32 * max(count, 1))
        _check(self._ctx, _lib.lib().dkg_fixed_base_batch(self._ctx, base, count, scalars, out))
        return out.raw[: 32 * count]

    def poly_eval_batch(self, coeffs: bytes, D: int, N: int, xs: List[int]) -> bytes:
        M = len(xs)
        arr = _carray(ctypes.c_uint32, M, xs)
        out = ctypes.create_string_buffer(32 * max(D * M, 1))
        _check(self._ctx, _lib.lib().dkg_poly_eval_batch(self._ctx, D, N, coeffs, M, arr, out))
        return out.raw[: 32 * D * M]

    def points_valid(self, points: bytes) -> bytes:
        count = len(points) // 32
        out = ctypes.create_string_buffer(max(count, 1))
        _check(self._ctx, _lib.lib().dkg_points_valid_batch(self._ctx, count, points, out))
        return out.raw[:count]

    # ---- round 1
    def share_gen(self, a: bytes, b: bytes, D: int, n: int, t: int):
        N = t + 1
        E, A = ctypes.create_string_buffer(32 * D * N), ctypes.create_string_buffer(32 * D * N)
        s, sp = ctypes.create_string_buffer(32 * D * n), ctypes.create_string_buffer(32 * D * n)
        _check(self._ctx, _lib.lib().dkg_share_gen(self._ctx, D, n, t, a, b, E, A, s, sp))
        return E.raw, A.raw, s.raw, sp.raw

    def share_gen_device(self, D: int, n: int, t: int, d_a: int, d_b: int, d_E: Optional[int], d_A: Optional[int],
                         d_s: int, d_sp: int):
        """dkg_share_gen on device buffers (pointers): compressed E/A [D][t+1][32], shares [D][n][32]."""
        vp = ctypes.c_void_p
        _check(self._ctx, _lib.lib().dkg_share_gen_device(self._ctx, D, n, t, vp(d_a), vp(d_b), vp(d_E), vp(d_A),
                                                           vp(d_s), vp(d_sp)))

    # ---- rounds 2 / 4
    def verify_pairs(self, n: int, t: int, rnd: int, d0: int, d1: int, C: bytes, s: bytes,
                     s_prime: Optional[bytes] = None) -> bytes:
        dec = ctypes.create_string_buffer(max((d1 - d0) * n, 1))
        _check(self._ctx, _lib.lib().dkg_verify_pairs(self._ctx, n, t, rnd, d0, d1, C, s, s_prime, dec))
        return dec.raw[: (d1 - d0) * n]

    def verify_receiver(self, n: int, t: int, rnd: int, j: int, C: bytes, s_col: bytes,
                        sp_col: Optional[bytes] = None) -> bytes:
        dec = ctypes.create_string_buffer(max(n, 1))
        _check(self._ctx, _lib.lib().dkg_verify_receiver(self._ctx, n, t, rnd, j, C, s_col, sp_col, dec))
        return dec.raw[:n]

    # ---- one party's view (chunked evaluation, receivers.hip)
    def set_receiver_chunk(self, chunk: int = 0):
        """Chunk length of commitment_eval / verify_receivers / party_round2: 0 automatic (receiver_plan),
        >= 1 forced.  Also the chunk of the wave evaluator (commitment_eval_pairs, complaint evaluation
        mode 4: pair_eval_shape), whose calls raise for a chunk that needs more than 64 lanes.  Outputs do
        not depend on it."""
        _check(self._ctx, _lib.lib().dkg_ctx_set_receiver_chunk(self._ctx, chunk))

    def last_receiver_chunk(self) -> int:
        return _lib.lib().dkg_ctx_last_receiver_chunk(self._ctx)

    def commitment_eval(self, D: int, t: int, js: Sequence[int], C: bytes):
        """(P, ok): P[m][i] = sum_k (js[m]+1)^k C_i[k] as M*D encodings, ok [D] = row i decodes (its P zero
        otherwise)."""
        M = len(js)
        arr = (ctypes.c_uint32 * max(M, 1))(*js)
        P = ctypes.create_string_buffer(max(32 * M * D, 1))
        ok = ctypes.create_string_buffer(max(D, 1))
        _check(self._ctx, _lib.lib().dkg_commitment_eval(self._ctx, D, t, M, arr, C, P, ok))
        return P.raw[: 32 * M * D], ok.raw[:D]

    def commitment_eval_pairs(self, D: int, t: int, rows: Sequence[int], js: Sequence[int], C: bytes):
        """(P, ok) for the (row, index) pairs (rows[p], js[p]), any order, repeats allowed: P[p] =
        sum_k (js[p]+1)^k C_rows[p][k] as len(rows) encodings, ok[p] = row rows[p] decodes (its P zero
        otherwise).  One wave per pair (pair_eval_shape under set_receiver_chunk); only the distinct rows
        named are decoded."""
        cnt = len(rows)
        if len(js) != cnt:
            raise ValueError("rows and js differ in length")
        ra = (ctypes.c_uint32 * max(cnt, 1))(*rows)
        ja = (ctypes.c_uint32 * max(cnt, 1))(*js)
        P = ctypes.create_string_buffer(max(32 * cnt, 1))
        ok = ctypes.create_string_buffer(max(cnt, 1))
        _check(self._ctx, _lib.lib().dkg_commitment_eval_pairs(self._ctx, D, t, cnt, ra, ja, C, P, ok))
        return P.raw[: 32 * cnt], ok.raw[:cnt]

    def verify_receivers(self, n: int, t: int, rnd: int, js: Sequence[int], C: bytes, s_cols: bytes,
                         sp_cols: Optional[bytes] = None, qualified: Optional[bytes] = None) -> bytes:
        """verify_receiver for the indices js (0-based) in one call: s_cols / sp_cols [M][n][32], decisions
        [M][n]; qualified [n] (round 4): 0 marks SKIPPED."""
        M = len(js)
        arr = (ctypes.c_uint32 * max(M, 1))(*js)
        dec = ctypes.create_string_buffer(max(M * n, 1))
        _check(self._ctx, _lib.lib().dkg_verify_receivers(self._ctx, n, t, rnd, M, arr, C, s_cols, sp_cols, qualified,
                                                           dec))
        return dec.raw[: M * n]

    def party_round2(self, n: int, t: int, j: int, E: bytes, e1_col: bytes, ct_col: bytes, sk: bytes,
                     w: Optional[bytes] = None) -> dict:
        """Round 2 of party j in full mode: e1_col, ct_col [n][2][32] addressed to j, sk its secret key, w
        [n][64] the proofs' nonces (None: no proofs).  Keys: s, s_prime, dec, complaints, r2_error, proofs."""
        s = ctypes.create_string_buffer(32 * n)
        sp = ctypes.create_string_buffer(32 * n)
        dec = ctypes.create_string_buffer(n)
        cnt = ctypes.c_int32(0)
        err = ctypes.c_uint8(0)
        prf = ctypes.create_string_buffer(192 * n) if w is not None else None
        _check(self._ctx, _lib.lib().dkg_party_round2(self._ctx, n, t, j, E, e1_col, ct_col, sk, w, s, sp, dec,
                                                       ctypes.byref(cnt), ctypes.byref(err), prf))
        return {"s": s.raw, "s_prime": sp.raw, "dec": dec.raw, "complaints": cnt.value, "r2_error": err.value,
                "proofs": prf.raw if prf is not None else None}

    # ---- hosted seats: one operator's party index in each of many ceremonies (k_seat_horner)
    @staticmethod
    def _seat_arrays(cer, js):
        S = len(cer)
        if len(js) != S:
            raise ValueError("cer and js differ in length")
        return S, (ctypes.c_uint32 * max(S, 1))(*cer), (ctypes.c_uint32 * max(S, 1))(*js)

    def commitment_eval_seats(self, B: int, n: int, t: int, cer: Sequence[int], js: Sequence[int], C: bytes):
        """(P, ok) for the seats (cer[p], js[p]) of B ceremonies of (n, t), C [B*n][t+1][32]: P[p][i] =
        sum_k (js[p]+1)^k C_{cer[p], i}[k] as S*n encodings, ok [S][n] = the row decodes (its P zero
        otherwise).  commitment_eval per seat in one call; only the ceremonies named are decoded."""
        S, ca, ja = self._seat_arrays(cer, js)
        P = ctypes.create_string_buffer(max(32 * S * n, 1))
        ok = ctypes.create_string_buffer(max(S * n, 1))
        _check(self._ctx, _lib.lib().dkg_commitment_eval_seats(self._ctx, B, n, t, S, ca, ja, C, P, ok))
        return P.raw[: 32 * S * n], ok.raw[: S * n]

    def verify_seats(self, B: int, n: int, t: int, rnd: int, cer: Sequence[int], js: Sequence[int], C: bytes,
                     s_cols: bytes, sp_cols: Optional[bytes] = None, qualified: Optional[bytes] = None) -> bytes:
        """verify_receivers with one index per seat, all seats in one call: s_cols / sp_cols [S][n][32],
        decisions [S][n]; qualified [B][n] (round 4): 0 marks SKIPPED for that ceremony's seats."""
        S, ca, ja = self._seat_arrays(cer, js)
        dec = ctypes.create_string_buffer(max(S * n, 1))
        _check(self._ctx, _lib.lib().dkg_verify_seats(self._ctx, B, n, t, rnd, S, ca, ja, C, s_cols, sp_cols, qualified,
                                                       dec))
        return dec.raw[: S * n]

    def party_round2_seats(self, B: int, n: int, t: int, cer: Sequence[int], js: Sequence[int], E: bytes,
                           e1_cols: bytes, ct_cols: bytes, sks: bytes, w: Optional[bytes] = None) -> dict:
        """party_round2 for every seat in one call: e1_cols, ct_cols [S][n][2][32], sks [S][32], w [S][n][64]
        (None: no proofs).  Keys: s, s_prime [S][n][32], dec [S][n], complaints [S], r2_error [S], proofs
        [S][n][192] or None."""
        S, ca, ja = self._seat_arrays(cer, js)
        s = ctypes.create_string_buffer(max(32 * S * n, 1))
        sp = ctypes.create_string_buffer(max(32 * S * n, 1))
        dec = ctypes.create_string_buffer(max(S * n, 1))
        cnt = (ctypes.c_int32 * max(S, 1))()
        err = ctypes.create_string_buffer(max(S, 1))
        prf = ctypes.create_string_buffer(max(192 * S * n, 1)) if w is not None else None
        _check(self._ctx, _lib.lib().dkg_party_round2_seats(self._ctx, B, n, t, S, ca, ja, E, e1_cols, ct_cols, sks, w,
                                                             s, sp, dec, cnt, err, prf))
        return {"s": s.raw[: 32 * S * n], "s_prime": sp.raw[: 32 * S * n], "dec": dec.raw[: S * n],
                "complaints": list(cnt[:S]), "r2_error": list(err.raw[:S]),
                "proofs": prf.raw[: 192 * S * n] if prf is not None else None}

    # ---- hosted seats deal round 1 (k_seat_enc_mul)
    def party_round1_seats(self, B: int, n: int, t: int, cer: Sequence[int], js: Sequence[int], a: bytes, b: bytes,
                           r: bytes, pk: bytes) -> dict:
        """Phases<Initialise>::init for every seat in one call: a, b [S][t+1][32] the seats' coefficients, r
        [S][n][2][32] their encryption randomness (w = 0 for s', 1 for s), pk [B][n][32] the ceremonies' sorted
        member keys.  Keys: E, A [S][t+1][32]; e1, ct [S][n][2][32]; s, s_prime [S][n][32]; own [S][2][32] =
        (s', s) at js[p].  Row p equals share_gen(D = 1) + encrypt_shares(D = 1) of seat p."""
        S, ca, ja = self._seat_arrays(cer, js)
        N = t + 1
        E, A = (ctypes.create_string_buffer(max(32 * S * N, 1)) for _ in range(2))
        e1, ct = (ctypes.create_string_buffer(max(64 * S * n, 1)) for _ in range(2))
        s, sp = (ctypes.create_string_buffer(max(32 * S * n, 1)) for _ in range(2))
        own = ctypes.create_string_buffer(max(64 * S, 1))
        _check(self._ctx, _lib.lib().dkg_party_round1_seats(self._ctx, B, n, t, S, ca, ja, a, b, r, pk, E, A, e1, ct, s,
                                                             sp, own))
        return {"E": E.raw[: 32 * S * N], "A": A.raw[: 32 * S * N], "e1": e1.raw[: 64 * S * n],
                "ct": ct.raw[: 64 * S * n], "s": s.raw[: 32 * S * n], "s_prime": sp.raw[: 32 * S * n],
                "own": own.raw[: 64 * S]}

    def set_seat_deal(self, mode: int):
        """K = pk_q r of party_round1_seats: 0 (default) automatic, 1 a radix-16 comb per key slot, 2 the joint
        radix-4 chain of both scalars.  Outputs do not depend on it."""
        _check(self._ctx, _lib.lib().dkg_ctx_set_seat_deal(self._ctx, mode))

    def last_seat_deal(self) -> int:
        """The route (1 or 2) the last party_round1_seats ran; 0 before the first."""
        return _lib.lib().dkg_ctx_last_seat_deal(self._ctx)

    def set_seat_eval(self, mode: int = 0, chunk: int = 0):
        """The evaluation of commitment_eval_seats / verify_seats / party_round2_seats: 0 (default) automatic
        by seat_eval_shape's rule, 1 the serial walk, 2 chunked with seat_eval_shape(.., chunk) (chunk 0: the
        rule's; a shape of one chunk runs the serial walk).  chunk must be 0 outside mode 2.  Outputs do not
        depend on it."""
        _check(self._ctx, _lib.lib().dkg_ctx_set_seat_eval(self._ctx, mode, chunk))

    def last_seat_eval(self) -> tuple:
        """(route, L) of the last seats call: route 1 serial (L = t + 1) or 2 chunked; (0, 0) before the first."""
        c = ctypes.c_int(0)
        mode = _lib.lib().dkg_ctx_last_seat_eval(self._ctx, ctypes.byref(c))
        return mode, c.value

    # ---- hosted seats through rounds 3-5 (k_seat_lagrange; the batch's complaint kernels)
    def complaints_verify_ceremonies(self, B: int, n: int, t: int, ceremony: Sequence[int], accusers: Sequence[int],
                                     accused: Sequence[int], pk: bytes, E: bytes, enc: bytes, proofs: bytes,
                                     fetched1: Optional[bytes] = None, want_qualified: bool = True):
        """complaints_verify for the complaints of B ceremonies in one call: (verdicts [C], qualified [B*n] or
        None).  ceremony 0-based, accusers / accused 1-based; pk [B][n][32], E [B*n][t+1][32], enc [C][128]."""
        C = len(ceremony)
        if len(accusers) != C or len(accused) != C:
            raise ValueError("ceremony, accusers and accused differ in length")
        res = _carray(ctypes.c_int32, C)
        q = ctypes.create_string_buffer(max(B * n, 1)) if want_qualified else None
        _check(self._ctx, _lib.lib().dkg_complaints_verify_ceremonies(
            self._ctx, B, n, t, C, _carray(ctypes.c_uint32, C, ceremony), _carray(ctypes.c_uint32, C, accusers),
            _carray(ctypes.c_uint32, C, accused), pk, E, None if fetched1 is None else bytes(fetched1), enc, proofs,
            res, q))
        return list(res)[:C], (list(q.raw[:B * n]) if q is not None else None)

    def complaints3_verify_ceremonies(self, B: int, n: int, t: int, ceremony: Sequence[int], accusers: Sequence[int],
                                      accused: Sequence[int], share: bytes, randomness: bytes, E: bytes, A: bytes,
                                      qualified: Optional[bytes] = None, fetched3: Optional[bytes] = None):
        """complaints3_verify for the round-4 complaints of B ceremonies in one call: (verdicts [C],
        reconstruct [B*n]).  qualified / fetched3 [B*n] (None = all 1)."""
        C = len(ceremony)
        if len(accusers) != C or len(accused) != C:
            raise ValueError("ceremony, accusers and accused differ in length")
        res = _carray(ctypes.c_int32, C)
        rec = ctypes.create_string_buffer(max(B * n, 1))
        _check(self._ctx, _lib.lib().dkg_complaints3_verify_ceremonies(
            self._ctx, B, n, t, C, _carray(ctypes.c_uint32, C, ceremony), _carray(ctypes.c_uint32, C, accusers),
            _carray(ctypes.c_uint32, C, accused), share, randomness, E, A,
            None if qualified is None else bytes(qualified), None if fetched3 is None else bytes(fetched3), res, rec))
        return list(res)[:C], list(rec.raw[:B * n])

    def party_round3_seats(self, B: int, n: int, t: int, cer: Sequence[int], js: Sequence[int], qualified: bytes,
                           s_cols: bytes, public: bool = True):
        """Phases<Phase2>::proceed per seat: (final_share, public_share), [S][32] each (public_share None
        without `public`); qualified [B][n], s_cols [S][n][32]."""
        S, ca, ja = self._seat_arrays(cer, js)
        fs = ctypes.create_string_buffer(max(32 * S, 1))
        ps = ctypes.create_string_buffer(max(32 * S, 1)) if public else None
        _check(self._ctx, _lib.lib().dkg_party_round3_seats(self._ctx, B, n, t, S, ca, ja, bytes(qualified), s_cols,
                                                             fs, ps))
        return fs.raw[: 32 * S], (ps.raw[: 32 * S] if ps is not None else None)

    def finalise_seats(self, B: int, n: int, t: int, cer: Sequence[int], js: Sequence[int], qualified: bytes,
                       reconstruct: bytes, A0: bytes, s_cols: bytes, disclosures=(), fetched3: Optional[bytes] = None,
                       r2_error=None, r4_error=None) -> "PartyFinalise":
        """Phases<Phase5>::finalise per seat (dkg_finalise_seats).  qualified, reconstruct [B][n]; A0 [B*n][32];
        s_cols [S][n][32] the seats' own columns; disclosures: (ceremony, sender, dealer, share) with sender /
        dealer 1-based, or a 4-tuple (ceremonies, senders, dealers, share bytes) of flat arrays; r2_error /
        r4_error [S] the seats' own.  PartyFinalise with one entry per seat."""
        S, ca, ja = self._seat_arrays(cer, js)
        if isinstance(disclosures, tuple) and len(disclosures) == 4 and isinstance(disclosures[3], (bytes, bytearray)):
            dc, dsnd, dd, dsh = disclosures
            dsh = bytes(dsh)
        else:
            disclosures = list(disclosures)
            dc, dsnd, dd = ([d[k] for d in disclosures] for k in range(3))
            dsh = b"".join(d[3] for d in disclosures)
        D5 = len(dc)
        if len(dsnd) != D5 or len(dd) != D5 or len(dsh) != 32 * D5:
            raise ValueError("the disclosure arrays differ in length")
        mask = lambda x: None if x is None else bytes(bytearray(x))  # noqa: E731
        mpk = ctypes.create_string_buffer(32 * max(S, 1))
        st = _carray(ctypes.c_int32, S)
        ri = _carray(ctypes.c_int32, S)
        arr = lambda v: _carray(ctypes.c_uint32, D5, v) if D5 else None  # noqa: E731
        _check(self._ctx, _lib.lib().dkg_finalise_seats(
            self._ctx, B, n, t, S, ca, ja, mask(qualified), mask(reconstruct), mask(fetched3), mask(r2_error),
            mask(r4_error), A0, s_cols, D5, arr(dc), arr(dsnd), arr(dd), dsh if D5 else None, mpk, st, ri))
        m = mpk.raw
        return PartyFinalise([m[32 * p:32 * p + 32] for p in range(S)], list(st)[:S], list(ri)[:S])

    # ---- public shares of every party from the broadcast commitments (k_commit_colsum)
    def commitment_sum(self, B: int, n: int, t: int, A: bytes, mask=None):
        """(S, ok) of dkg_commitment_sum: S[c][k] = the sum over the dealers i with mask[c][i] (None: all) of
        A_{c,i}[k] as B*(t+1) encodings, A [B*n][t+1][32]; ok [B] = 0 (and row c zero) where a masked row does not
        decode."""
        N = t + 1
        S = ctypes.create_string_buffer(max(32 * B * N, 1))
        ok = ctypes.create_string_buffer(max(B, 1))
        _check(self._ctx, _lib.lib().dkg_commitment_sum(self._ctx, B, n, t, A,
                                                         None if mask is None else bytes(bytearray(mask)), S, ok))
        return S.raw[: 32 * B * N], ok.raw[:B]

    def public_shares(self, B: int, n: int, t: int, A: bytes, qualified, js: Sequence[int], reconstruct=None,
                      disclosures=(), fetched3=None, want_sum: bool = False) -> "PublicShares":
        """The public shares g s_j of the parties js (0-based; one list for all B ceremonies) from public data
        (dkg_public_shares): A [B*n][t+1][32] the round-3 vectors, qualified / reconstruct [B][n] (reconstruct
        None = none), fetched3 [B*n] (None = all present); disclosures: the phase-5 shares in the two forms
        finalise_seats takes.  PublicShares: V [B][M][32], status and which [B*M], S [B][t+1][32] with want_sum."""
        M = len(js)
        if isinstance(disclosures, tuple) and len(disclosures) == 4 and isinstance(disclosures[3], (bytes, bytearray)):
            dc, dsnd, dd, dsh = disclosures
            dsh = bytes(dsh)
        else:
            disclosures = list(disclosures)
            dc, dsnd, dd = ([d[k] for d in disclosures] for k in range(3))
            dsh = b"".join(d[3] for d in disclosures)
        D5 = len(dc)
        if len(dsnd) != D5 or len(dd) != D5 or len(dsh) != 32 * D5:
            raise ValueError("the disclosure arrays differ in length")
        mask = lambda x: None if x is None else bytes(bytearray(x))  # noqa: E731
        arr = lambda v: _carray(ctypes.c_uint32, D5, v) if D5 else None  # noqa: E731
        N = t + 1
        V = ctypes.create_string_buffer(max(32 * B * M, 1))
        st = _carray(ctypes.c_int32, B * M)
        wh = _carray(ctypes.c_int32, B * M)
        S = ctypes.create_string_buffer(max(32 * B * N, 1)) if want_sum else None
        _check(self._ctx, _lib.lib().dkg_public_shares(
            self._ctx, B, n, t, A, mask(qualified), mask(reconstruct), mask(fetched3), M,
            _carray(ctypes.c_uint32, M, js), D5, arr(dc), arr(dsnd), arr(dd), dsh if D5 else None, V, st, wh, S))
        return PublicShares(V.raw[: 32 * B * M], list(st)[: B * M], list(wh)[: B * M],
                            S.raw[: 32 * B * N] if S is not None else None)

    def set_public_share_slab(self, rows: int = 0):
        """Rows of A that commitment_sum / public_shares decode at a time: 0 (default) automatic.  Outputs do
        not depend on it."""
        _check(self._ctx, _lib.lib().dkg_ctx_set_public_share_slab(self._ctx, rows))

    # ---- whole ceremony
    def _ceremony_out(self, n, t, big):
        N = t + 1
        bufs = {}
        o = CeremonyOut()
        sizes = {"qualified": n, "r2_error": n, "r4_error": n, "complaints2": 4 * n, "reconstruct": n}
        if big:
            sizes.update({"E": 32 * n * N, "A": 32 * n * N, "s": 32 * n * n, "s_prime": 32 * n * n,
                          "dec2": n * n, "dec4": n * n, "final_share": 32 * n, "public_share": 32 * n})
        for k, v in sizes.items():
            bufs[k] = ctypes.create_string_buffer(v)
            setattr(o, k, ctypes.cast(bufs[k], ctypes.c_void_p))
        return o, bufs

    def _result(self, n, t, o, bufs, big):
        import struct
        r = CeremonyResult(
            n=n, t=t, mpk=bytes(o.mpk), qualified=list(bufs["qualified"].raw[:n]),
            r2_error=list(bufs["r2_error"].raw[:n]), r4_error=list(bufs["r4_error"].raw[:n]),
            complaints2=list(struct.unpack(f"<{n}i", bufs["complaints2"].raw[: 4 * n])),
            reconstruct=list(bufs["reconstruct"].raw[:n]), n_qualified=o.n_qualified,
            phase4_error=o.phase4_error,
            ms={"round1": o.ms_round1, "round2": o.ms_round2, "round3": o.ms_round3, "round4": o.ms_round4,
                "finalise": o.ms_finalise, "total": o.ms_total})
        if big:
            for k in ("E", "A", "s", "s_prime", "dec2", "dec4", "final_share", "public_share"):
                setattr(r, k, bufs[k].raw)
        return r

    def _ceremony_call(self, fn, n, t, args, tail=(), big=True, given=None):
        """One ceremony entry point, fn(ctx, n, t, *args, out, *tail), as a CeremonyResult.  given: the
        big fields that the caller supplied, {name: bytes}: null in the out struct, so not copied back,
        and put on the result as they came."""
        given = given or {}
        o, bufs = self._ceremony_out(n, t, big)
        for k in given:
            setattr(o, k, None)
        _check(self._ctx, fn(self._ctx, n, t, *args, ctypes.byref(o), *tail))
        r = self._result(n, t, o, bufs, big)
        for k, v in given.items():
            setattr(r, k, v)
        return r

    def ceremony(self, a: bytes, b: bytes, n: int, t: int) -> CeremonyResult:
        return self._ceremony_call(_lib.lib().dkg_ceremony_run, n, t, (a, b))

    def ceremony_verify(self, E: bytes, A: bytes, s: bytes, s_prime: bytes, n: int, t: int) -> CeremonyResult:
        return self._ceremony_call(_lib.lib().dkg_ceremony_verify, n, t, (E, A, s, s_prime),
                                   given={"E": E, "A": A, "s": s, "s_prime": s_prime})

    def ceremony_verify_fetched(self, E: bytes, A: bytes, s: bytes, s_prime: bytes, fetched1: bytes,
                                fetched3: bytes, n: int, t: int) -> CeremonyResult:
        """ceremony_verify after the broadcast intake (MembersFetchedState1/3::from_broadcast):
        fetched1[i] / fetched3[i] = 0 for a dealer whose phase-1 / phase-3 broadcast is absent or
        malformed (see dkg_amd.broadcast)."""
        return self._ceremony_call(_lib.lib().dkg_ceremony_verify_fetched, n, t,
                                   (E, A, s, s_prime, fetched1, fetched3),
                                   given={"E": E, "A": A, "s": s, "s_prime": s_prime})

    def ceremony_device(self, d_a: int, d_b: int, n: int, t: int) -> CeremonyResult:
        """d_a, d_b: device pointers (e.g. torch tensor .data_ptr()) to [n][t+1][32] scalars."""
        vp = ctypes.c_void_p
        return self._ceremony_call(_lib.lib().dkg_ceremony_run_device, n, t, (vp(d_a), vp(d_b)), big=False)

    # ---- full (encrypted-share) mode
    def member_keys(self, master: bytes, ceremony: int, n: int):
        """Seeded member communication keys, sorted by public key (party q+1 owns sk[q]): (sk, pk)."""
        sk, pk = ctypes.create_string_buffer(32 * n), ctypes.create_string_buffer(32 * n)
        _check(self._ctx, _lib.lib().dkg_member_keys(self._ctx, master, ceremony, n, sk, pk))
        return sk.raw, pk.raw

    def encrypt_shares(self, pk: bytes, s: bytes, s_prime: bytes, r: bytes, D: int, n: int):
        e1, ct = ctypes.create_string_buffer(64 * D * n), ctypes.create_string_buffer(64 * D * n)
        _check(self._ctx, _lib.lib().dkg_encrypt_shares(self._ctx, D, n, pk, s, s_prime, r, e1, ct))
        return e1.raw, ct.raw

    def decrypt_shares(self, sk: bytes, e1: bytes, ct: bytes, D: int, n: int):
        s, sp, ok = (ctypes.create_string_buffer(32 * D * n), ctypes.create_string_buffer(32 * D * n),
                     ctypes.create_string_buffer(2 * D * n))
        _check(self._ctx, _lib.lib().dkg_decrypt_shares(self._ctx, D, n, sk, e1, ct, s, sp, ok))
        return s.raw, sp.raw, ok.raw

    def enc_randomness_device(self, master: bytes, ceremony0: int, B: int, d0: int, D: int, n: int, t: int, d_r: int):
        _check(self._ctx, _lib.lib().dkg_enc_randomness_device(self._ctx, master, ceremony0, B, d0, D, n, t,
                                                                ctypes.c_void_p(d_r)))

    def ceremony_full_device(self, d_a: int, d_b: int, d_r: int, sk: bytes, pk: bytes, n: int, t: int):
        vp = ctypes.c_void_p
        return self._ceremony_call(_lib.lib().dkg_ceremony_run_full_device, n, t, (vp(d_a), vp(d_b), vp(d_r), sk, pk),
                                   big=False)

    def ceremony_verify_full(self, E: bytes, A: bytes, e1: bytes, ct: bytes, sk: bytes, n: int, t: int):
        return self._ceremony_call(_lib.lib().dkg_ceremony_verify_full, n, t, (E, A, e1, ct, sk),
                                   given={"E": E, "A": A})

    # ---- full mode for batches of ceremonies (key arrays [B][n][32], rows c*n + i = dealer i of ceremony c)
    def member_keys_batch(self, master: bytes, ceremony0: int, B: int, n: int):
        """member_keys of ceremonies ceremony0 .. ceremony0 + B-1 in one launch: (sk, pk), each [B][n][32]."""
        sk, pk = ctypes.create_string_buffer(max(32 * B * n, 1)), ctypes.create_string_buffer(max(32 * B * n, 1))
        _check(self._ctx, _lib.lib().dkg_member_keys_batch(self._ctx, master, ceremony0, B, n, sk, pk))
        return sk.raw[:32 * B * n], pk.raw[:32 * B * n]

    def encrypt_shares_batch(self, pk: bytes, s: bytes, s_prime: bytes, r: bytes, B: int, n: int):
        """encrypt_shares per ceremony (recipient q of ceremony c under pk[c][q]): (e1, ct)."""
        size = 64 * B * n * n
        e1, ct = ctypes.create_string_buffer(max(size, 1)), ctypes.create_string_buffer(max(size, 1))
        _check(self._ctx, _lib.lib().dkg_encrypt_shares_batch(self._ctx, B, n, pk, s, s_prime, r, e1, ct))
        return e1.raw[:size], ct.raw[:size]

    def decrypt_shares_batch(self, sk: bytes, e1: bytes, ct: bytes, B: int, n: int):
        """decrypt_shares per ceremony with sk [B][n][32]: (s, s_prime, ok)."""
        V = B * n
        s, sp, ok = (ctypes.create_string_buffer(max(32 * V * n, 1)), ctypes.create_string_buffer(max(32 * V * n, 1)),
                     ctypes.create_string_buffer(max(2 * V * n, 1)))
        _check(self._ctx, _lib.lib().dkg_decrypt_shares_batch(self._ctx, B, n, sk, e1, ct, s, sp, ok))
        return s.raw[:32 * V * n], sp.raw[:32 * V * n], ok.raw[:2 * V * n]

    def set_batch_full_chunk(self, ceremonies: int):
        """Ceremonies per chunk of the batched hybrid stage (0: automatic).  Outputs do not depend on it."""
        _check(self._ctx, _lib.lib().dkg_ctx_set_batch_full_chunk(self._ctx, ceremonies))

    def batch_full_phase_times(self) -> dict:
        """Device ms of the last batched full-mode call's hybrid kernels, summed over its chunks."""
        names = ("enc_decode", "enc_tab", "enc_e1", "enc_mul", "enc_encode", "enc_sym",
                 "dec_decode", "dec_mul", "dec_encode", "dec_sym")
        out = {}
        for nm in names:
            v = _lib.lib().dkg_ctx_phase_ms(self._ctx, f"bfull.{nm}".encode())
            if v >= 0:
                out[nm] = v
        return out

    # ---- complaint proofs (broadcast.rs)
    def misbehaviour_prove(self, sk: bytes, enc: bytes, w: bytes) -> bytes:
        """ProofOfMisbehaviour::generate for B = len(sk) // 32 complaints: proofs [B][192]."""
        B = len(sk) // 32
        out = ctypes.create_string_buffer(max(192 * B, 1))
        _check(self._ctx, _lib.lib().dkg_misbehaviour_prove(self._ctx, B, sk, enc, w, out))
        return out.raw[:192 * B]

    def complaint1_verify(self, t: int, accusers: List[int], pk: bytes, enc: bytes, E: bytes, proofs: bytes):
        B = len(accusers)
        acc = _carray(ctypes.c_uint32, B, accusers)
        res = _carray(ctypes.c_int32, B)
        _check(self._ctx, _lib.lib().dkg_complaint1_verify(self._ctx, B, t, acc, pk, enc, E, proofs, res))
        return list(res)[:B]

    def complaint3_verify(self, t: int, accusers: List[int], share: bytes, randomness: bytes, E: bytes, A: bytes):
        B = len(accusers)
        acc = _carray(ctypes.c_uint32, B, accusers)
        res = _carray(ctypes.c_int32, B)
        _check(self._ctx, _lib.lib().dkg_complaint3_verify(self._ctx, B, t, acc, share, randomness, E, A, res))
        return list(res)[:B]

    # ---- round-2 complaints as device batches, and the qualified set they prove (committee.rs:370-398)
    def set_complaint_eval(self, mode: int):
        """How complaints_verify / complaints3_verify evaluate P_i(j): 0 automatic, 1 per-pair Horner, 2
        difference tables, 4 one wave per (row, index) item (pair_eval_shape under set_receiver_chunk).
        3 and anything above 4 raise.  Outputs do not depend on it."""
        _check(self._ctx, _lib.lib().dkg_ctx_set_complaint_eval(self._ctx, mode))

    def complaints_prove(self, sk: bytes, enc: bytes, w: bytes) -> bytes:
        """ProofOfMisbehaviour::generate for C = len(sk) // 32 complaints on the device: proofs [C][192],
        byte-identical to misbehaviour_prove."""
        C = len(sk) // 32
        out = ctypes.create_string_buffer(max(192 * C, 1))
        _check(self._ctx, _lib.lib().dkg_complaints_prove(self._ctx, C, sk, enc, w, out))
        return out.raw[:192 * C]

    def complaints_verify(self, n: int, t: int, accusers: Sequence[int], accused: Sequence[int], pk: bytes, E: bytes,
                          enc: bytes, proofs: bytes, fetched1: Optional[bytes] = None):
        """compute_qualified_set over the broadcast complaints of one ceremony: (verdicts, qualified).
        accusers / accused 1-based; enc [C][128] = what the ACCUSED broadcast to the accuser."""
        C = len(accusers)
        acc = _carray(ctypes.c_uint32, C, accusers)
        acd = _carray(ctypes.c_uint32, C, accused)
        res = _carray(ctypes.c_int32, C)
        q = ctypes.create_string_buffer(max(n, 1))
        _check(self._ctx, _lib.lib().dkg_complaints_verify(self._ctx, n, t, C, acc, acd, pk, E, fetched1, enc, proofs,
                                                            res, q))
        return list(res)[:C], list(q.raw[:n])

    def ceremony_verify_full_complaints(self, E: bytes, A: bytes, e1: bytes, ct: bytes, sk: bytes, pk: bytes,
                                        accusers: Sequence[int], accused: Sequence[int], proofs: bytes, n: int,
                                        t: int):
        """ceremony_verify_full with the reference's rule for the qualified set: a dealer is cleared only
        by a complaint that verifies.  Returns (CeremonyResult, verdicts, dissent)."""
        C = len(accusers)
        res, dis = _carray(ctypes.c_int32, C), _carray(ctypes.c_int32, n)
        r = self._ceremony_call(
            _lib.lib().dkg_ceremony_verify_full_complaints, n, t,
            (E, A, e1, ct, sk, pk, C, _carray(ctypes.c_uint32, C, accusers), _carray(ctypes.c_uint32, C, accused), proofs),
            (res, dis), given={"E": E, "A": A})
        return r, list(res)[:C], list(dis)[:n]

    # ---- round-4 complaints as a device batch, and the reconstructable set they prove (committee.rs:625-688)
    def complaints3_verify(self, n: int, t: int, accusers: Sequence[int], accused: Sequence[int], share: bytes,
                           randomness: bytes, E: bytes, A: bytes, qualified: Optional[bytes] = None,
                           fetched3: Optional[bytes] = None):
        """Phases<Phase4>::proceed's loop over the broadcast round-4 complaints of one ceremony:
        (verdicts, reconstruct).  accusers / accused 1-based; share / randomness [C][32] as disclosed."""
        C = len(accusers)
        acc = _carray(ctypes.c_uint32, C, accusers)
        acd = _carray(ctypes.c_uint32, C, accused)
        res = _carray(ctypes.c_int32, C)
        rec = ctypes.create_string_buffer(max(n, 1))
        _check(self._ctx, _lib.lib().dkg_complaints3_verify(
            self._ctx, n, t, C, acc, acd, share, randomness, E, A,
            None if qualified is None else bytes(qualified), None if fetched3 is None else bytes(fetched3), res, rec))
        return list(res)[:C], list(rec.raw[:n])

    def ceremony_verify_fetched_proven(self, E: bytes, A: bytes, s: bytes, s_prime: bytes, fetched1: bytes,
                                       fetched3: bytes, accusers4: Sequence[int], accused4: Sequence[int],
                                       share4: bytes, randomness4: bytes, n: int, t: int) -> ProvenResult:
        """ceremony_verify_fetched whose reconstruct follows the proven round-4 complaints."""
        C4 = len(accusers4)
        res = _carray(ctypes.c_int32, C4)
        st, ri = ctypes.c_int32(), ctypes.c_int32()
        r = self._ceremony_call(
            _lib.lib().dkg_ceremony_verify_fetched_proven, n, t,
            (E, A, s, s_prime, bytes(fetched1), bytes(fetched3), C4, _carray(ctypes.c_uint32, C4, accusers4),
             _carray(ctypes.c_uint32, C4, accused4), share4, randomness4),
            (res, ctypes.byref(st), ctypes.byref(ri)), given={"E": E, "A": A, "s": s, "s_prime": s_prime})
        return ProvenResult(r, list(res)[:C4], st.value, ri.value)

    def ceremony_verify_full_proven(self, E: bytes, A: bytes, e1: bytes, ct: bytes, sk: bytes, pk: bytes,
                                    accusers: Sequence[int], accused: Sequence[int], proofs: bytes,
                                    accusers4: Sequence[int], accused4: Sequence[int], share4: bytes,
                                    randomness4: bytes, n: int, t: int,
                                    fetched3: Optional[bytes] = None) -> ProvenResult:
        """ceremony_verify_full_complaints whose reconstruct follows the proven round-4 complaints."""
        C, C4 = len(accusers), len(accusers4)
        res, res4, dis = _carray(ctypes.c_int32, C), _carray(ctypes.c_int32, C4), _carray(ctypes.c_int32, n)
        st, ri = ctypes.c_int32(), ctypes.c_int32()
        r = self._ceremony_call(
            _lib.lib().dkg_ceremony_verify_full_proven, n, t,
            (E, A, e1, ct, sk, pk, C, _carray(ctypes.c_uint32, C, accusers), _carray(ctypes.c_uint32, C, accused), proofs,
             None if fetched3 is None else bytes(fetched3), C4, _carray(ctypes.c_uint32, C4, accusers4),
             _carray(ctypes.c_uint32, C4, accused4), share4, randomness4),
            (res, dis, res4, ctypes.byref(st), ctypes.byref(ri)), given={"E": E, "A": A})
        return ProvenResult(r, list(res4)[:C4], st.value, ri.value, list(res)[:C], list(dis)[:n])

    def dealer_coefficients_device(self, master: bytes, ceremony0: int, B: int, d0: int, D: int, t: int,
                                   d_a: int, d_b: int):
        """dkg_dealer_coeffs on the GPU for B ceremonies: rows [B*D][t+1][32] at device pointers."""
        vp = ctypes.c_void_p
        _check(self._ctx, _lib.lib().dkg_dealer_coeffs_device(self._ctx, master, ceremony0, B, d0, D, t, vp(d_a),
                                                               vp(d_b)))

    # ---- one rank of a dealer-sharded ceremony: rounds 2-5 of its dealers [d0, d1).  The d_* are device
    # pointers (e.g. torch tensor .data_ptr())
    def _shard_call(self, fn, n, t, d0, d1, args) -> float:
        """One sharded entry point, fn(ctx, n, t, d0, d1, *args, &ms_total): the call's device time in ms."""
        ms = ctypes.c_double()
        _check(self._ctx, fn(self._ctx, n, t, d0, d1, *args, ctypes.byref(ms)))
        return ms.value

    def ceremony_shard_device(self, n, t, d0, d1, d_a, d_b, d_dec2, d_dec4, d_A0, d_partial) -> float:
        return self._shard_call(_lib.lib().dkg_ceremony_shard_device, n, t, d0, d1,
                                (d_a, d_b, d_dec2, d_dec4, d_A0, d_partial))

    def ceremony_shard_verify_device(self, n, t, d0, d1, d_E, d_A, d_s, d_sp, d_dec2, d_dec4, d_A0,
                                     d_partial) -> float:
        """Rounds 2-5 of this rank's dealers [d0, d1) on received broadcasts (device pointers)."""
        return self._shard_call(_lib.lib().dkg_ceremony_shard_verify_device, n, t, d0, d1,
                                (d_E, d_A, d_s, d_sp, d_dec2, d_dec4, d_A0, d_partial))

    def ceremony_shard_full_device(self, n, t, d0, d1, d_a, d_b, d_r, sk: bytes, pk: bytes, d_dec2, d_dec4, d_A0,
                                   d_partial, d_e1: Optional[int] = None, d_ct: Optional[int] = None) -> float:
        """ceremony_shard_device in full (encrypted-share) mode: this rank's dealers' shares encrypted to
        the n member keys (d_r: device [D][n][2][32] randomness; sk, pk host [n][32]), decrypted by all n
        receivers, and checked.  d_e1 / d_ct (device [D][n][2][32], optional) receive the ciphertexts."""
        return self._shard_call(_lib.lib().dkg_ceremony_shard_full_device, n, t, d0, d1,
                                (d_a, d_b, d_r, sk, pk, d_e1, d_ct, d_dec2, d_dec4, d_A0, d_partial))

    def ceremony_shard_verify_full_device(self, n, t, d0, d1, d_E, d_A, d_e1, d_ct, sk: bytes, d_dec2, d_dec4, d_A0,
                                          d_partial) -> float:
        """ceremony_shard_verify_device on received ciphertexts d_e1, d_ct (device [D][n][2][32])."""
        return self._shard_call(_lib.lib().dkg_ceremony_shard_verify_full_device, n, t, d0, d1,
                                (d_E, d_A, d_e1, d_ct, sk, d_dec2, d_dec4, d_A0, d_partial))

    # the sharded calls that decide by the proven complaints (each rank verifies those against its own dealers)
    def ceremony_shard_verify_proven_device(self, n, t, d0, d1, d_E, d_A, d_s, d_sp, accusers4: Sequence[int],
                                            accused4: Sequence[int], share4: bytes, randomness4: bytes, d_dec2, d_dec4,
                                            d_A0, d_partial, flag_rows: int, d_flags, fetched1: Optional[bytes] = None,
                                            fetched3: Optional[bytes] = None):
        """ceremony_shard_verify_device whose round 4 follows the proven complaints.  The WHOLE broadcast
        round-4 complaint list goes in (1-based indices); returns (ms, verdict4) with COMPLAINT_NOT_OWNED
        for the complaints against other ranks' dealers.  d_flags: device [flag_rows] u32 flag words
        (flag_rows = shard_rows(n, world_size)); fetched1 / fetched3: the rank's rows' intake masks."""
        C4 = len(accusers4)
        res4 = _carray(ctypes.c_int32, C4)
        ms = self._shard_call(_lib.lib().dkg_ceremony_shard_verify_proven_device, n, t, d0, d1, (
            d_E, d_A, d_s, d_sp, _opt(fetched1), _opt(fetched3), C4, _carray(ctypes.c_uint32, C4, accusers4),
            _carray(ctypes.c_uint32, C4, accused4), share4, randomness4, d_dec2, d_dec4, d_A0, d_partial, flag_rows,
            d_flags, res4))
        return ms, list(res4)[:C4]

    def ceremony_shard_verify_full_proven_device(self, n, t, d0, d1, d_E, d_A, d_e1, d_ct, sk: bytes, pk: bytes,
                                                 accusers: Sequence[int], accused: Sequence[int], proofs: bytes,
                                                 accusers4: Sequence[int], accused4: Sequence[int], share4: bytes,
                                                 randomness4: bytes, d_dec2, d_dec4, d_A0, d_partial, flag_rows: int,
                                                 d_flags, d_dissent=None, fetched1: Optional[bytes] = None,
                                                 fetched3: Optional[bytes] = None):
        """ceremony_shard_verify_full_device with both rounds decided by the proven complaints: returns
        (ms, verdict, verdict4).  d_dissent: device [n] i32, the rank's dissent partial (optional)."""
        C, C4 = len(accusers), len(accusers4)
        res, res4 = _carray(ctypes.c_int32, C), _carray(ctypes.c_int32, C4)
        ms = self._shard_call(_lib.lib().dkg_ceremony_shard_verify_full_proven_device, n, t, d0, d1, (
            d_E, d_A, d_e1, d_ct, sk, pk, _opt(fetched1), _opt(fetched3), C, _carray(ctypes.c_uint32, C, accusers),
            _carray(ctypes.c_uint32, C, accused), proofs, C4, _carray(ctypes.c_uint32, C4, accusers4),
            _carray(ctypes.c_uint32, C4, accused4), share4, randomness4, d_dec2, d_dec4, d_A0, d_partial, flag_rows,
            d_flags, d_dissent, res, res4))
        return ms, list(res)[:C], list(res4)[:C4]

    def last_complaint_eval(self) -> int:
        """Where the last sharded proven call took P_i(j) from: 3 its own pass, 1 Horner, 2 tables, 12 both."""
        return _lib.lib().dkg_ctx_last_complaint_eval(self._ctx)

    def shard_combine_proven_device(self, n: int, t: int, world_size: int, d_pack2_g: int, d_pack4_g: int,
                                    d_flags_g: int, d_dissent_g: Optional[int] = None, full: bool = True,
                                    d_dec2: Optional[int] = None, d_dec4: Optional[int] = None):
        """Combine step of the sharded proven calls (dkg_shard_combine_proven_device) from the gathered
        packed rows, flag words [ws][R] and dissent partials [ws][n]: (ShardOutcome, dissent or None,
        finalise_status, recovery_index)."""
        q, r2e, rc, r4e = (ctypes.create_string_buffer(max(n, 1)) for _ in range(4))
        c = _carray(ctypes.c_int32, n)
        o = _lib.ShardOutcome(ctypes.cast(q, ctypes.c_void_p), ctypes.cast(c, ctypes.c_void_p),
                              ctypes.cast(r2e, ctypes.c_void_p), ctypes.cast(rc, ctypes.c_void_p),
                              ctypes.cast(r4e, ctypes.c_void_p), 0, 0)
        dis = _carray(ctypes.c_int32, n) if d_dissent_g is not None else None
        st, ri = ctypes.c_int32(), ctypes.c_int32()
        vp = ctypes.c_void_p
        _check(self._ctx, _lib.lib().dkg_shard_combine_proven_device(
            self._ctx, n, t, world_size, vp(d_pack2_g), vp(d_pack4_g), vp(d_flags_g), vp(d_dissent_g),
            int(bool(full)), vp(d_dec2), vp(d_dec4), ctypes.byref(o), dis, ctypes.byref(st), ctypes.byref(ri)))
        out = ShardOutcome(list(q.raw[:n]), list(c)[:n], list(r2e.raw[:n]), list(rc.raw[:n]), list(r4e.raw[:n]),
                           o.n_qualified, bool(o.phase4_error))
        return out, (None if dis is None else list(dis)[:n]), st.value, ri.value

    def set_key_comb(self, mode: int):
        """Comb of the recipient keys behind full mode's K = pk_q r: 0 (default) radix 2^10 tables, the
        sharded full calls choosing by key_comb_choice; 1 radix 2^10 everywhere; 2 radix 16 everywhere.
        Outputs do not depend on it."""
        _check(self._ctx, _lib.lib().dkg_ctx_set_key_comb(self._ctx, mode))

    def last_key_comb(self) -> int:
        """The kind (1 or 2) the last single-ceremony encryption used."""
        return _lib.lib().dkg_ctx_last_key_comb(self._ctx)

    def set_comb_build(self, mode: int):
        """Builder of the radix-2^BITS comb tables (dkg_ctx_set_comb_build): 0 automatic, 1 one thread per
        entry, 2 chained.  Governs every comb built afterwards and drops the cached caller-base and member-key
        combs.  Outputs do not depend on it."""
        _check(self._ctx, _lib.lib().dkg_ctx_set_comb_build(self._ctx, mode))

    def last_comb_build(self) -> int:
        """The builder (1 or 2) the last comb build ran; 0 before the first."""
        return _lib.lib().dkg_ctx_last_comb_build(self._ctx)

    def last_comb_build_ms(self) -> float:
        """Device time of the last comb build, ms."""
        return _lib.lib().dkg_ctx_last_comb_build_ms(self._ctx)

    def comb_entries(self, kind: int, base: Optional[bytes], window: int, first: int, count: int) -> bytes:
        """dkg_comb_entries: a fresh build of the comb of `base` (None = the generator) with the current
        builder; entries d = first + 1 .. first + count of `window` as count x 96 bytes, the canonical
        encodings of y + x, y - x, 2dxy."""
        out = ctypes.create_string_buffer(max(96 * count, 1))
        b = None if base is None else bytes(base)
        if b is not None and len(b) != 32:
            raise ValueError("base must be 32 bytes")
        _check(self._ctx, _lib.lib().dkg_comb_entries(self._ctx, kind, b, window, first, count,
                                                      ctypes.cast(out, ctypes.c_void_p)))
        return out.raw[:96 * count]

    def ceremony_shard_recon_device(self, n, t, d0, d1, qualified, reconstruct, d_s: Optional[int], d_terms: int,
                                    r2_error=None, r4_error=None) -> bool:
        """After the exchange: replace the terms of this rank's reconstructed dealers by g * a_i0
        interpolated over the disclosing final parties' shares (no r2 / r4 error; d_s None = the
        last shard call's rows).  Returns True when fewer than t final parties disclose
        (InsufficientSharesForRecovery for everyone: no mpk; the terms are untouched)."""
        vp = ctypes.c_void_p
        opt = lambda m: None if m is None else bytes(bytearray(m))  # noqa: E731
        fails = ctypes.c_int32(0)
        _check(self._ctx, _lib.lib().dkg_ceremony_shard_recon_device(
            self._ctx, n, t, d0, d1, bytes(bytearray(qualified)), bytes(bytearray(reconstruct)), opt(r2_error),
            opt(r4_error), vp(d_s), vp(d_terms), ctypes.byref(fails)))
        return bool(fails.value)

    def finalise_parties(self, n: int, t: int, qualified, reconstruct, A0: bytes, s: bytes, r2_error=None,
                         r4_error=None, disclosed=None) -> "PartyFinalise":
        """Phases<Phase5>::finalise as every party runs it (committee.rs:726-805), with optional
        per-party earlier failures and missing phase-5 disclosures (dkg_finalise_parties)."""
        mpk = ctypes.create_string_buffer(32 * max(n, 1))
        st = _carray(ctypes.c_int32, n)
        ri = _carray(ctypes.c_int32, n)
        mask = lambda x: None if x is None else bytes(bytearray(x))  # noqa: E731
        _check(self._ctx, _lib.lib().dkg_finalise_parties(
            self._ctx, n, t, mask(qualified), mask(reconstruct), mask(r2_error), mask(r4_error), mask(disclosed),
            A0, s, mpk, st, ri))
        m = mpk.raw
        return PartyFinalise([m[32 * p:32 * p + 32] for p in range(n)], list(st)[:n], list(ri)[:n])

    def shard_combine_device(self, n: int, t: int, world_size: int, d_dec2_g: int, d_dec4_g: int,
                             d_dec2: Optional[int] = None, d_dec4: Optional[int] = None,
                             packed: bool = False, arrays: bool = False) -> "ShardOutcome":
        """Combine step of the sharded run (dkg_shard_combine_device): the common round-2/4 outcome
        from the all-gathered [ws][R][n] decision blocks (device pointers; with packed, the
        [ws][R][packed_row_words(n)] bitmaps of dkg_shard_combine_packed_device); d_dec2 / d_dec4
        optionally receive the compacted [n][n] matrices (dec4 with SKIPPED rows).  arrays: the
        per-party outcomes as numpy arrays (uint8 / int32) instead of lists -- no per-element
        conversion on the multi-GPU driver's path."""
        q, r2e, rc, r4e = (ctypes.create_string_buffer(max(n, 1)) for _ in range(4))
        c = _carray(ctypes.c_int32, n)
        o = _lib.ShardOutcome(ctypes.cast(q, ctypes.c_void_p), ctypes.cast(c, ctypes.c_void_p),
                              ctypes.cast(r2e, ctypes.c_void_p), ctypes.cast(rc, ctypes.c_void_p),
                              ctypes.cast(r4e, ctypes.c_void_p), 0, 0)
        vp = ctypes.c_void_p
        fn = _lib.lib().dkg_shard_combine_packed_device if packed else _lib.lib().dkg_shard_combine_device
        _check(self._ctx, fn(self._ctx, n, t, world_size, vp(d_dec2_g), vp(d_dec4_g), vp(d_dec2), vp(d_dec4),
                             ctypes.byref(o)))
        if arrays:
            import numpy as np

            u8 = lambda b: np.frombuffer(b.raw, dtype=np.uint8, count=n).copy()  # noqa: E731
            return ShardOutcome(u8(q), np.frombuffer(c, dtype=np.int32, count=n).copy(), u8(r2e), u8(rc), u8(r4e),
                                o.n_qualified, bool(o.phase4_error))
        return ShardOutcome(list(q.raw[:n]), list(c)[:n], list(r2e.raw[:n]), list(rc.raw[:n]), list(r4e.raw[:n]),
                            o.n_qualified, bool(o.phase4_error))

    def decisions_pack_device(self, rows: int, nvalid: int, n: int, d0: int, d_dec: int, d_packed: int):
        """Raw decision rows of dealers d0.. (device [nvalid][n] bytes) -> the packed bitmaps the ranks
        all-gather (device [rows][packed_row_words(n)] u32; dkg_decisions_pack_device).  Raises if a
        row holds values the encoding cannot carry."""
        vp = ctypes.c_void_p
        _check(self._ctx, _lib.lib().dkg_decisions_pack_device(self._ctx, rows, nvalid, n, d0, vp(d_dec),
                                                                vp(d_packed)))

    def shard_finalise_device(self, n: int, t: int, world_size: int, d_terms_g: int, d_partials_g: int, qualified,
                              phase4_error: bool, d_final_share: int, d_public_share: Optional[int] = None) -> bytes:
        """Finalise of the sharded run (dkg_shard_finalise_device): final shares (and public shares)
        into device buffers; returns the mpk (zero when phase4_error)."""
        mpk = ctypes.create_string_buffer(32)
        vp = ctypes.c_void_p
        _check(self._ctx, _lib.lib().dkg_shard_finalise_device(
            self._ctx, n, t, world_size, vp(d_terms_g), vp(d_partials_g), bytes(bytearray(qualified)),
            int(bool(phase4_error)), vp(d_final_share), vp(d_public_share), mpk))
        return mpk.raw

    def scalar_sum_device(self, rows: int, n: int, d_in: int, d_mask: Optional[int], d_out: int):
        """out[j] = sum over rows r with mask[r] of in[r][j] mod l (device pointers)."""
        vp = ctypes.c_void_p
        _check(self._ctx, _lib.lib().dkg_scalar_sum_device(self._ctx, rows, n, vp(d_in), vp(d_mask), vp(d_out)))

    def point_sum_device(self, count: int, d_points: int, d_mask: Optional[int], d_out: int):
        """out = sum of the compressed points[c] with mask[c] (device pointers)."""
        vp = ctypes.c_void_p
        _check(self._ctx, _lib.lib().dkg_point_sum_device(self._ctx, count, vp(d_points), vp(d_mask), vp(d_out)))


class _ShardView(Backend):
    """A shard's dkg_ctx inside a MultiBackend (owned by the multi-device context: close is a no-op)."""

    def __init__(self, ctx, owner):
        self._ctx, self.h, self._owner = ctx, None, owner

    def close(self):
        self._ctx = None


class MultiBackend:
    """Several GPUs driven from ONE process (dkg_multi_*, SURVEY.md section 8(b) threading row): the
    ceremony sharded by dealer over `devices`, exchanged by peer copies into devices[0], combined and
    finalised there.  Results equal Backend.ceremony / ceremony_verify's except that E, A, s,
    s_prime are not returned (they stay on the shards' devices).  A device may repeat."""

    def __init__(self, devices):
        L = _lib.lib()
        devs = (ctypes.c_int * len(devices))(*devices)
        h = ctypes.c_void_p()
        rc = L.dkg_multi_create(devs, len(devices), ctypes.byref(h))
        if rc != _lib.DKG_OK:
            raise DkgError(rc, f"dkg_multi_create(devices={list(devices)}) failed (are gfx950 GPUs visible?)")
        self._m = h
        self.devices = list(devices)
        self.h: Optional[bytes] = None

    def close(self):
        if self._m:
            _lib.lib().dkg_multi_destroy(self._m)
            self._m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != _lib.DKG_OK:
            raise DkgError(rc, _lib.lib().dkg_multi_last_error(self._m).decode())

    def __len__(self):
        return _lib.lib().dkg_multi_size(self._m)

    def shard(self, i: int) -> Backend:
        """Shard i's context, for its tuning knobs (set_split, set_streams, ...)."""
        ctx = _lib.lib().dkg_multi_ctx(self._m, i)
        if not ctx:
            raise DkgError(_lib.DKG_E_ARG, f"no shard {i}")
        return _ShardView(ctypes.c_void_p(ctx), self)

    def phase_ms(self) -> dict:
        L = _lib.lib()
        return {k: L.dkg_multi_phase_ms(self._m, k.encode())
                for k in ("shard_max", "shard_min", "exchange", "combine", "recon", "finalise")}

    def env_init(self, threshold: int, nr_members: int, ck_gen_bytes: bytes = CK_DEFAULT) -> bytes:
        out = ctypes.create_string_buffer(32)
        self._check(_lib.lib().dkg_multi_env_init(self._m, threshold, nr_members, ck_gen_bytes, len(ck_gen_bytes),
                                                  out))
        self.h = out.raw
        return out.raw

    def _out(self, n, t):
        o, bufs = Backend._ceremony_out(None, n, t, True)
        for k in ("E", "A", "s", "s_prime"):
            setattr(o, k, None)
        return o, bufs

    def _result(self, n, t, o, bufs):
        r = Backend._result(None, n, t, o, bufs, False)
        for k in ("dec2", "dec4", "final_share", "public_share"):
            setattr(r, k, bufs[k].raw)
        return r

    def _ceremony_call(self, fn, n, t, args, tail=()) -> CeremonyResult:
        """One multi-device entry point, fn(m, n, t, *args, out, *tail), as a CeremonyResult."""
        o, bufs = self._out(n, t)
        self._check(fn(self._m, n, t, *args, ctypes.byref(o), *tail))
        return self._result(n, t, o, bufs)

    def _pointers(self, per_shard):
        return (ctypes.c_void_p * len(self.devices))(*per_shard)

    def ceremony(self, a: bytes, b: bytes, n: int, t: int) -> CeremonyResult:
        return self._ceremony_call(_lib.lib().dkg_multi_ceremony_run, n, t, (a, b))

    def ceremony_device(self, d_as, d_bs, n: int, t: int) -> CeremonyResult:
        """d_as[i], d_bs[i]: device pointers on devices[i] to shard i's dealers' coefficients."""
        return self._ceremony_call(_lib.lib().dkg_multi_ceremony_run_device, n, t,
                                   (self._pointers(d_as), self._pointers(d_bs)))

    def ceremony_verify(self, E: bytes, A: bytes, s: bytes, s_prime: bytes, n: int, t: int) -> CeremonyResult:
        return self._ceremony_call(_lib.lib().dkg_multi_ceremony_verify, n, t, (E, A, s, s_prime))

    # ---- full (encrypted-share) mode: each shard encrypts, decrypts and checks its dealers' rows
    def ceremony_full(self, a: bytes, b: bytes, r: bytes, sk: bytes, pk: bytes, n: int, t: int) -> CeremonyResult:
        """r: host [n][n][2][32] encryption randomness (enc_randomness); sk, pk: member_keys."""
        return self._ceremony_call(_lib.lib().dkg_multi_ceremony_run_full, n, t, (a, b, r, sk, pk))

    def ceremony_full_device(self, d_as, d_bs, d_rs, sk: bytes, pk: bytes, n: int, t: int) -> CeremonyResult:
        """d_as[i], d_bs[i], d_rs[i]: device pointers on devices[i] to shard i's coefficients and randomness."""
        return self._ceremony_call(_lib.lib().dkg_multi_ceremony_run_full_device, n, t,
                                   (self._pointers(d_as), self._pointers(d_bs), self._pointers(d_rs), sk, pk))

    def ceremony_verify_full(self, E: bytes, A: bytes, e1: bytes, ct: bytes, sk: bytes, n: int, t: int) -> CeremonyResult:
        return self._ceremony_call(_lib.lib().dkg_multi_ceremony_verify_full, n, t, (E, A, e1, ct, sk))

    # ---- the proven-complaint rule: each shard verifies the complaints against its own dealers
    def ceremony_verify_proven(self, E: bytes, A: bytes, s: bytes, s_prime: bytes, fetched1: Optional[bytes],
                               fetched3: Optional[bytes], accusers4: Sequence[int], accused4: Sequence[int],
                               share4: bytes, randomness4: bytes, n: int, t: int) -> ProvenResult:
        """Backend.ceremony_verify_fetched_proven over the shards (fetched1 / fetched3 None = all present)."""
        C4 = len(accusers4)
        res4 = _carray(ctypes.c_int32, C4)
        st, ri = ctypes.c_int32(), ctypes.c_int32()
        r = self._ceremony_call(
            _lib.lib().dkg_multi_ceremony_verify_proven, n, t,
            (E, A, s, s_prime, _opt(fetched1), _opt(fetched3), C4, _carray(ctypes.c_uint32, C4, accusers4),
             _carray(ctypes.c_uint32, C4, accused4), share4, randomness4),
            tail=(res4, ctypes.byref(st), ctypes.byref(ri)))
        return ProvenResult(r, list(res4)[:C4], st.value, ri.value)

    def ceremony_verify_full_proven(self, E: bytes, A: bytes, e1: bytes, ct: bytes, sk: bytes, pk: bytes,
                                    accusers: Sequence[int], accused: Sequence[int], proofs: bytes,
                                    accusers4: Sequence[int], accused4: Sequence[int], share4: bytes,
                                    randomness4: bytes, n: int, t: int,
                                    fetched3: Optional[bytes] = None) -> ProvenResult:
        """Backend.ceremony_verify_full_proven over the shards."""
        C, C4 = len(accusers), len(accusers4)
        res, res4, dis = _carray(ctypes.c_int32, C), _carray(ctypes.c_int32, C4), _carray(ctypes.c_int32, n)
        st, ri = ctypes.c_int32(), ctypes.c_int32()
        r = self._ceremony_call(
            _lib.lib().dkg_multi_ceremony_verify_full_proven, n, t,
            (E, A, e1, ct, sk, pk, C, _carray(ctypes.c_uint32, C, accusers), _carray(ctypes.c_uint32, C, accused),
             proofs, _opt(fetched3), C4, _carray(ctypes.c_uint32, C4, accusers4),
             _carray(ctypes.c_uint32, C4, accused4), share4, randomness4),
            tail=(res, dis, res4, ctypes.byref(st), ctypes.byref(ri)))
        return ProvenResult(r, list(res4)[:C4], st.value, ri.value, list(res)[:C], list(dis)[:n])


@dataclass
class ShardOutcome:
    """The common outcome of a sharded ceremony (dkg_shard_combine_device), identical on every rank."""
    qualified: List[int]
    complaints2: List[int]
    r2_error: List[int]
    reconstruct: List[int]
    r4_error: List[int]
    n_qualified: int
    phase4_error: bool


def shard_range(n: int, world_size: int, rank: int):
    """Dealers [d0, d1) of `rank` (dkg_shard_range: contiguous, sizes differ by at most one)."""
    d0, d1 = ctypes.c_size_t(), ctypes.c_size_t()
    _lib.lib().dkg_shard_range(n, world_size, rank, ctypes.byref(d0), ctypes.byref(d1))
    return d0.value, d1.value


def device_pci_bus_id(device: int) -> str:
    """PCI bus id ("dddd:bb:dd.f") of HIP device `device` (dkg_device_pci_bus_id)."""
    b = ctypes.create_string_buffer(64)
    rc = _lib.lib().dkg_device_pci_bus_id(device, b, len(b))
    if rc != _lib.DKG_OK:
        raise DkgError(rc, f"dkg_device_pci_bus_id({device}) failed")
    return b.value.decode()


def shard_rows(n: int, world_size: int) -> int:
    """Padded per-rank block height R of the all-gathers (dkg_shard_rows)."""
    return _lib.lib().dkg_shard_rows(n, world_size)


def owning_rank(n: int, world_size: int, dealer: int) -> int:
    """The rank whose shard_range holds the 0-based `dealer`."""
    r = min(world_size - 1, dealer * world_size // n)
    while shard_range(n, world_size, r)[1] <= dealer:
        r += 1
    while shard_range(n, world_size, r)[0] > dealer:
        r -= 1
    return r


def merge_verdicts(per_rank: Sequence[Sequence[int]]) -> List[int]:
    """The ceremony's verdict list from the ranks' arrays of a sharded proven call: the element-wise
    maximum (COMPLAINT_NOT_OWNED is below every real code, and exactly one rank owns each complaint).
    Raises if some complaint is owned by nobody."""
    out = [max(col) for col in zip(*per_rank)] if per_rank else []
    if any(v == _lib.COMPLAINT_NOT_OWNED for v in out):
        raise ValueError("a complaint is owned by no rank")
    return out


def key_comb_choice(keys: int, items_per_key: int, cached10: bool = False, cached16: bool = False) -> int:
    """The cost rule of the sharded full calls (dkg_key_comb_choice): 1 = radix 2^10 tables, 2 = radix-16
    combs, whichever builds (unless cached) and multiplies `items_per_key` items per key faster."""
    return _lib.lib().dkg_key_comb_choice(keys, items_per_key, int(bool(cached10)), int(bool(cached16)))


def comb_geometry(kind: int) -> dict:
    """dkg_comb_geometry (host only): kind 0 the shared bases' comb, kind 1 the member keys'.  Keys: bits,
    windows, entries (per window), chunk (consecutive entries per thread of the chained builder)."""
    b, w = ctypes.c_int(), ctypes.c_int()
    e, c = ctypes.c_uint32(), ctypes.c_uint32()
    rc = _lib.lib().dkg_comb_geometry(kind, ctypes.byref(b), ctypes.byref(w), ctypes.byref(e), ctypes.byref(c))
    if rc != _lib.DKG_OK:
        raise _lib.DkgError(rc, "comb_geometry")
    return {"bits": b.value, "windows": w.value, "entries": e.value, "chunk": c.value}


def receiver_plan(n: int, t: int, x: int, chunk: int = 0) -> dict:
    """dkg_receiver_plan_for (host only): the chunk length and fold stages the one-party evaluation runs
    for receiver index x (1-based).  Keys: chunk, stages, arity [stages], mult [stages] (ints),
    cost_us (the rule's estimate)."""
    p = _lib.ReceiverPlan()
    L = _lib.lib()
    rc = L.dkg_receiver_plan_for(n, t, x, chunk, ctypes.byref(p))
    if rc != _lib.DKG_OK:
        raise _lib.DkgError(rc, "receiver_plan")
    return {"chunk": p.chunk, "stages": p.stages, "arity": list(p.arity[: p.stages]),
            "mult": [int.from_bytes(bytes(p.mult[s]), "little") for s in range(p.stages)],
            "cost_us": L.dkg_receiver_plan_cost_us(n, t, x, ctypes.byref(p))}


def pair_eval_shape(t: int, chunk: int = 0) -> dict:
    """dkg_pair_eval_shape (host only): the shape one wave runs per (row, index) pair at threshold t.
    Keys: chunk (L), lanes, stages.  chunk 0 automatic; raises for a forced chunk needing > 64 lanes."""
    v = [ctypes.c_uint32() for _ in range(3)]
    rc = _lib.lib().dkg_pair_eval_shape(t, chunk, *[ctypes.byref(x) for x in v])
    if rc != _lib.DKG_OK:
        raise _lib.DkgError(rc, "pair_eval_shape")
    return {"chunk": v[0].value, "lanes": v[1].value, "stages": v[2].value}


def seat_pack(n: int, js: Sequence[int]) -> dict:
    """dkg_seat_pack (host only): how the seats with party indices js (0-based) of ceremonies of n parties
    share the waves of the seats calls.  Keys: width, per_wave, tiles, wave_of [S], slot_of [S], waves."""
    S = len(js)
    ja = (ctypes.c_uint32 * max(S, 1))(*js)
    wave_of = (ctypes.c_uint32 * max(S, 1))()
    slot_of = (ctypes.c_uint32 * max(S, 1))()
    v = [ctypes.c_uint32() for _ in range(4)]
    rc = _lib.lib().dkg_seat_pack(n, S, ja, ctypes.byref(v[0]), ctypes.byref(v[1]), ctypes.byref(v[2]), wave_of, slot_of,
                                  ctypes.byref(v[3]))
    if rc != _lib.DKG_OK:
        raise _lib.DkgError(rc, "seat_pack")
    return {"width": v[0].value, "per_wave": v[1].value, "tiles": v[2].value, "wave_of": list(wave_of[:S]),
            "slot_of": list(slot_of[:S]), "waves": v[3].value}


def seat_eval_shape(n: int, t: int, waves: int, x_max: int, chunk: int = 0) -> dict:
    """dkg_seat_eval_shape (host only): the shape the seats calls evaluate `waves` waves of seat_pack in, the
    largest index being x_max (1-based).  Keys: chunk (L), chunks (G), stages, scratch_bytes, constants (the
    rule's: dkg_seat_eval_constants).  chunk 0 automatic; chunks == 1 is the serial walk."""
    v = [ctypes.c_uint32() for _ in range(3)]
    sb = ctypes.c_uint64()
    L = _lib.lib()
    rc = L.dkg_seat_eval_shape(n, t, waves, x_max, chunk, *[ctypes.byref(x) for x in v], ctypes.byref(sb))
    if rc != _lib.DKG_OK:
        raise _lib.DkgError(rc, "seat_eval_shape")
    c = (ctypes.c_double * 6)()
    L.dkg_seat_eval_constants(c)
    return {"chunk": v[0].value, "chunks": v[1].value, "stages": v[2].value, "scratch_bytes": sb.value,
            "constants": dict(zip(("launch_us", "op_latency_us", "lane_op_us", "serial_op_latency_us",
                                   "chunked_setup_us", "margin"), c))}


def seat_enc_digits(k: int) -> List[int]:
    """dkg_seat_enc_digits (host only): the signed radix-4 digits, window 0 first, that party_round1_seats'
    joint chain walks for the scalar k < 2^255, as the kernel's own routine computes them."""
    if k < 0 or k >= 1 << 256:
        raise _lib.DkgError(_lib.DKG_E_ARG, "seat_enc_digits")
    d = (ctypes.c_int8 * 128)()
    w = ctypes.c_int(0)
    rc = _lib.lib().dkg_seat_enc_digits(k.to_bytes(32, "little"), d, ctypes.byref(w))
    if rc != _lib.DKG_OK:
        raise _lib.DkgError(rc, "seat_enc_digits")
    return list(d[: w.value])


def seat_finalise_status(n: int, t: int, p: int, qualified, reconstruct, points: Sequence[int], a_present=None,
                         r2_error: bool = False, r4_error: bool = False):
    """dkg_seat_finalise_status (host only): (status, recovery_index) of seat p (0-based) from what it holds:
    qualified, reconstruct [n]; points[i] = the points held for dealer i (its own included); a_present [n]
    (None = all): dealer i's A_i0 was fetched and decodes.  The rule finalise_seats executes per seat."""
    mask = lambda x: None if x is None else bytes(bytearray(x))  # noqa: E731
    idx = ctypes.c_int32(-1)
    rc = _lib.lib().dkg_seat_finalise_status(n, t, p, mask(qualified), mask(reconstruct), mask(a_present),
                                             (ctypes.c_uint32 * max(n, 1))(*points), int(bool(r2_error)),
                                             int(bool(r4_error)), ctypes.byref(idx))
    if rc < 0:
        raise _lib.DkgError(rc, "seat_finalise_status")
    return rc, idx.value


def public_share_status(n: int, qualified, reconstruct, j: int, disclosures=(), a_present=None):
    """dkg_public_share_status (host only): (status, which) of the public share of party j (0-based) of one
    ceremony: qualified, reconstruct [n] (reconstruct None = none); disclosures: the (sender, dealer) pairs, 1-based,
    of the phase-5 shares at hand; a_present [n] (None = all): dealer i's round-3 vector was fetched and decodes.
    DKG_PS_NO_COMMITMENT first (which = the lowest used dealer that is absent), then DKG_PS_NO_DISCLOSURE (the lowest
    reconstructed dealer j did not disclose), else DKG_PS_OK and -1: what public_shares reports per (ceremony, j)."""
    mask = lambda x: None if x is None else bytes(bytearray(x))  # noqa: E731
    disclosures = list(disclosures)
    D5 = len(disclosures)
    which = ctypes.c_int32(-1)
    rc = _lib.lib().dkg_public_share_status(
        n, mask(qualified), mask(reconstruct), mask(a_present), j, D5,
        _carray(ctypes.c_uint32, D5, [d[0] for d in disclosures]) if D5 else None,
        _carray(ctypes.c_uint32, D5, [d[1] for d in disclosures]) if D5 else None, ctypes.byref(which))
    if rc < 0:
        raise _lib.DkgError(rc, "public_share_status")
    return rc, which.value


def seat_disclosures(qualified, reconstruct, s_col: bytes, t: Optional[int] = None):
    """What Phases<Phase4>::proceed (committee.rs:625-688) leaves a seat to broadcast (host only): (shares,
    phase4_error).  shares[i] = the seat's share of dealer i (32 bytes of s_col [n][32]) for the reconstructed
    dealers and None for the others -- BroadcastPhase5's Vec<Option<share>> -- or None as a whole with
    phase4_error, when the party broadcasts nothing (:673-677).  phase4_error needs the threshold t; without
    it it reads None and the shares are returned unconditionally."""
    n = len(qualified)
    if len(reconstruct) != n or len(s_col) != 32 * n:
        raise ValueError("qualified, reconstruct and s_col differ in length")
    if any(r and not q for q, r in zip(qualified, reconstruct)):
        raise ValueError("only qualified members are reconstructed (committee.rs:639)")
    err = None if t is None else sum(map(bool, qualified)) - sum(map(bool, reconstruct)) <= t
    if err:
        return None, True
    return [s_col[32 * i:32 * i + 32] if reconstruct[i] else None for i in range(n)], err


def receiver_plan_constants() -> dict:
    """The rule's fitted constants (dkg_receiver_plan_constants)."""
    c = (ctypes.c_double * 5)()
    _lib.lib().dkg_receiver_plan_constants(c)
    return dict(zip(("launch_us", "op_latency_us", "lane_op_us", "serial_op_latency_us", "chunked_setup_us"), c))


def key_comb_constants() -> dict:
    """The rule's constants (dkg_key_comb_constants)."""
    c = (ctypes.c_double * 6)()
    _lib.lib().dkg_key_comb_constants(c)
    return dict(zip(("build10_floor_us", "build10_us_per_key", "mul10_ns_per_item", "build16_floor_us",
                     "build16_us_per_key", "mul16_ns_per_item"), c))


def packed_row_words(n: int) -> int:
    """u32 words of one packed decision row (dkg_packed_row_words: ceil(n/32) ACCEPT-bit words + a kind word)."""
    return _lib.lib().dkg_packed_row_words(n)


@dataclass
class BatchResult:
    """Outputs of B independent ceremonies (row c*n + i = party i of ceremony c)."""
    B: int
    n: int
    t: int
    mpk: List[bytes]
    n_qualified: List[int]
    phase4_error: bytes
    qualified: bytes
    r2_error: bytes
    r4_error: bytes
    complaints2: "Int32s"  # list-like: indexing, slices (lists), iteration, == with a list
    reconstruct: bytes
    final_share: Optional[bytes]
    public_share: Optional[bytes]
    dec2: Optional[bytes]
    dec4: Optional[bytes]
    ms: dict
    s: Optional[bytes] = None        # ceremony_batch_verify_full: the decrypted shares [B*n][n][32]
    s_prime: Optional[bytes] = None

    def ceremony(self, c: int) -> dict:
        """The outputs of ceremony c in the layout of a single CeremonyResult."""
        n = self.n
        r = slice(c * n, (c + 1) * n)
        d = {"mpk": self.mpk[c], "n_qualified": self.n_qualified[c], "phase4_error": self.phase4_error[c],
             "qualified": list(self.qualified[r]),
             "r2_error": list(self.r2_error[r]), "r4_error": list(self.r4_error[r]),
             "complaints2": self.complaints2[r],
             "reconstruct": list(self.reconstruct[r])}
        for k in ("final_share", "public_share"):
            v = getattr(self, k)
            d[k] = v[32 * n * c:32 * n * (c + 1)] if v is not None else None
        for k in ("dec2", "dec4"):
            v = getattr(self, k)
            d[k] = v[n * n * c:n * n * (c + 1)] if v is not None else None
        return d


def _batch_out(B, n, big):
    V = B * n
    sizes = {"mpk": 32 * B, "n_qualified": 4 * B, "phase4_error": B, "qualified": V, "r2_error": V, "r4_error": V,
             "complaints2": 4 * V,
             "reconstruct": V}
    if big:
        sizes.update({"final_share": 32 * V, "public_share": 32 * V, "dec2": V * n, "dec4": V * n})
    o = BatchOut()
    bufs = {}
    for k, v in sizes.items():
        bufs[k] = ctypes.create_string_buffer(max(v, 1))
        setattr(o, k, ctypes.cast(bufs[k], ctypes.c_void_p))
    return o, bufs


class Int32s(Sequence):
    """Little-endian int32 rows of a batch output, converted to Python ints only where read: a
    10,000-ceremony batch holds 640,000 of them, and building the whole list up front costs more
    host time than the ceremonies' round 3.  A read-only Sequence (len, indexing, slices -> list,
    iteration, `in`, index, count, == against any sequence); tolist() / list(x) for a list (JSON,
    concatenation).  Unhashable, like the list it stands for."""

    def __init__(self, raw: bytes):
        self._mv = memoryview(raw).cast("i")

    def __len__(self):
        return len(self._mv)

    def __getitem__(self, i):
        return self._mv[i].tolist() if isinstance(i, slice) else self._mv[i]

    def __iter__(self):
        return iter(self._mv.tolist())

    def __eq__(self, other):
        try:
            return self._mv.tolist() == list(other)
        except TypeError:
            return NotImplemented

    __hash__ = None

    def __add__(self, other):
        return self._mv.tolist() + list(other)

    def __repr__(self):
        return f"Int32s({self._mv.tolist()!r})" if len(self) <= 16 else f"Int32s(<{len(self)} values>)"

    def tolist(self):
        return self._mv.tolist()


def _batch_result(B, n, t, o, bufs):
    import struct
    V = B * n
    g = lambda k, size: bufs[k].raw[:size] if k in bufs else None  # noqa: E731
    mpk = bufs["mpk"].raw  # one copy (each .raw access copies the whole buffer)
    return BatchResult(
        B=B, n=n, t=t, mpk=[mpk[32 * c:32 * c + 32] for c in range(B)],
        n_qualified=list(struct.unpack(f"<{B}i", bufs["n_qualified"].raw[:4 * B])),
        phase4_error=g("phase4_error", B),
        qualified=g("qualified", V), r2_error=g("r2_error", V), r4_error=g("r4_error", V),
        complaints2=Int32s(bufs["complaints2"].raw[:4 * V]),
        reconstruct=g("reconstruct", V), final_share=g("final_share", 32 * V), public_share=g("public_share", 32 * V),
        dec2=g("dec2", V * n), dec4=g("dec4", V * n),
        ms={"round1": o.ms_round1, "checks": o.ms_checks, "round3": o.ms_round3, "finalise": o.ms_finalise,
            "total": o.ms_total})


def _batch_call(be, fn, B, n, t, args, tail=(), big=True, cached=False):
    """One batch entry point, fn(ctx, B, n, t, *args, out, *tail), as a BatchResult.  cached: the output
    buffers are kept on the backend for the next batch of the same shape (the result holds copies)."""
    key = (B, n, big)
    cache = getattr(be, "_batch_bufs", None) if cached else None
    if cache is None or cache[0] != key:
        cache = (key,) + _batch_out(B, n, big)
        if cached:
            be._batch_bufs = cache
    o, bufs = cache[1], cache[2]
    _check(be.ctx, fn(be.ctx, B, n, t, *args, ctypes.byref(o), *tail))
    return _batch_result(B, n, t, o, bufs)


def _batch_call_shares(be, fn, B, n, t, args, tail=()):
    """_batch_call for the full verify entry points, fn(.., out, s_out, s_prime_out, *tail): the result
    also carries the decrypted s / s_prime [B*n][n][32]."""
    size = 32 * B * n * n
    s, sp = ctypes.create_string_buffer(max(size, 1)), ctypes.create_string_buffer(max(size, 1))
    r = _batch_call(be, fn, B, n, t, args, (s, sp) + tuple(tail))
    r.s, r.s_prime = s.raw[:size], sp.raw[:size]
    return r


def ceremony_batch_device(be: "Backend", B: int, n: int, t: int, d_a: int, d_b: int, big: bool = False) -> BatchResult:
    """B honest ceremonies from device coefficients [B*n][t+1][32] (dkg_ceremony_batch_device).  The
    output buffers are kept on the backend for the next batch of the same shape (the result holds
    copies): a 10,000-ceremony batch no longer allocates and zeroes ~5 MB of host buffers per call."""
    vp = ctypes.c_void_p
    return _batch_call(be, _lib.lib().dkg_ceremony_batch_device, B, n, t, (vp(d_a), vp(d_b)), big=big, cached=True)


def ceremony_batch_verify(be: "Backend", B: int, n: int, t: int, E: bytes, A: bytes, s: bytes,
                          s_prime: bytes) -> BatchResult:
    """Receiver side of B ceremonies from (possibly tampered) broadcast values (dkg_ceremony_batch_verify)."""
    return _batch_call(be, _lib.lib().dkg_ceremony_batch_verify, B, n, t, (E, A, s, s_prime))


def ceremony_batch_full_device(be: "Backend", B: int, n: int, t: int, d_a: int, d_b: int, d_r: int, sk: bytes,
                               pk: bytes, big: bool = False) -> BatchResult:
    """B honest full-mode ceremonies (dkg_ceremony_batch_full_device): device coefficients d_a, d_b
    [B*n][t+1][32], encryption randomness d_r [B*n][n][2][32] (enc_randomness_device(master, c0, B, 0, n, n,
    t, d_r)), sk / pk = member_keys_batch output.  Output buffers are kept on the backend as in
    ceremony_batch_device."""
    vp = ctypes.c_void_p
    return _batch_call(be, _lib.lib().dkg_ceremony_batch_full_device, B, n, t, (vp(d_a), vp(d_b), vp(d_r), sk, pk),
                       big=big, cached=True)


def ceremony_batch_verify_full(be: "Backend", B: int, n: int, t: int, E: bytes, A: bytes, e1: bytes, ct: bytes,
                               sk: bytes) -> BatchResult:
    """Receiver side of B full-mode ceremonies from (possibly tampered) broadcast values
    (dkg_ceremony_batch_verify_full); the result also carries the decrypted s / s_prime."""
    return _batch_call_shares(be, _lib.lib().dkg_ceremony_batch_verify_full, B, n, t, (E, A, e1, ct, sk))


@dataclass
class BatchProvenResult:
    """A batch whose ceremonies follow the PROVEN complaints (ceremony_batch_verify_proven,
    ceremony_batch_verify_full_proven).  `ceremony`, `accused*` as given; verdict4 / verdict in input
    order; finalise_status, recovery_index per ceremony as ProvenResult's; full mode adds the round-1
    complaints' verdict and dissent [B*n].  ceremony(c) is one ceremony's view: the fields of
    BatchResult.ceremony(c) plus its own verdicts (in their relative order), dissent and status."""
    result: BatchResult
    ceremony4: List[int]
    verdict4: List[int]
    finalise_status: List[int]
    recovery_index: List[int]
    ceremony2: Optional[List[int]] = None
    verdict: Optional[List[int]] = None
    dissent: Optional[List[int]] = None

    def ceremony(self, c: int) -> dict:
        n = self.result.n
        d = self.result.ceremony(c)
        d["verdict4"] = [v for g, v in zip(self.ceremony4, self.verdict4) if g == c]
        d["finalise_status"], d["recovery_index"] = self.finalise_status[c], self.recovery_index[c]
        if self.verdict is not None:
            d["verdict"] = [v for g, v in zip(self.ceremony2, self.verdict) if g == c]
            d["dissent"] = self.dissent[c * n:(c + 1) * n]
            sz = 32 * n * n
            d["s"], d["s_prime"] = self.result.s[sz * c:sz * (c + 1)], self.result.s_prime[sz * c:sz * (c + 1)]
        return d


def _opt(b):
    return None if b is None else bytes(b)


def ceremony_batch_verify_proven(be: "Backend", B: int, n: int, t: int, E: bytes, A: bytes, s: bytes, s_prime: bytes,
                                 ceremony4: Sequence[int], accusers4: Sequence[int], accused4: Sequence[int],
                                 share4: bytes, randomness4: bytes, fetched1: Optional[bytes] = None,
                                 fetched3: Optional[bytes] = None) -> BatchProvenResult:
    """Backend.ceremony_verify_fetched_proven for every ceremony of a batch
    (dkg_ceremony_batch_verify_proven): complaint c belongs to ceremony4[c] (0-based), accusers4 /
    accused4 are 1-based within it; any order.  fetched1 / fetched3 [B*n], None = all present."""
    C4 = len(accusers4)
    res4 = _carray(ctypes.c_int32, C4)
    st, ri = _carray(ctypes.c_int32, B), _carray(ctypes.c_int32, B)
    u32 = ctypes.c_uint32
    r = _batch_call(
        be, _lib.lib().dkg_ceremony_batch_verify_proven, B, n, t,
        (E, A, s, s_prime, _opt(fetched1), _opt(fetched3), C4, _carray(u32, C4, ceremony4),
         _carray(u32, C4, accusers4), _carray(u32, C4, accused4), share4, randomness4), (res4, st, ri))
    return BatchProvenResult(r, list(ceremony4), list(res4)[:C4], list(st)[:B], list(ri)[:B])


def ceremony_batch_verify_full_proven(be: "Backend", B: int, n: int, t: int, E: bytes, A: bytes, e1: bytes, ct: bytes,
                                      sk: bytes, pk: bytes, ceremony: Sequence[int], accusers: Sequence[int],
                                      accused: Sequence[int], proofs: bytes, ceremony4: Sequence[int],
                                      accusers4: Sequence[int], accused4: Sequence[int], share4: bytes,
                                      randomness4: bytes, fetched3: Optional[bytes] = None) -> BatchProvenResult:
    """Backend.ceremony_verify_full_proven for every ceremony of a batch
    (dkg_ceremony_batch_verify_full_proven): sk, pk [B][n][32]; the round-1 complaints (ceremony,
    accusers, accused, proofs [C][192]) and the round-4 complaints (ceremony4, ...) as flat lists over
    the batch.  The result also carries the decrypted s / s_prime."""
    C, C4 = len(accusers), len(accusers4)
    res, res4, dis = _carray(ctypes.c_int32, C), _carray(ctypes.c_int32, C4), _carray(ctypes.c_int32, B * n)
    st, ri = _carray(ctypes.c_int32, B), _carray(ctypes.c_int32, B)
    u32 = ctypes.c_uint32
    r = _batch_call_shares(
        be, _lib.lib().dkg_ceremony_batch_verify_full_proven, B, n, t,
        (E, A, e1, ct, sk, pk, C, _carray(u32, C, ceremony), _carray(u32, C, accusers), _carray(u32, C, accused),
         proofs, _opt(fetched3), C4, _carray(u32, C4, ceremony4), _carray(u32, C4, accusers4),
         _carray(u32, C4, accused4), share4, randomness4), (res, dis, res4, st, ri))
    return BatchProvenResult(r, list(ceremony4), list(res4)[:C4], list(st)[:B], list(ri)[:B], list(ceremony),
                             list(res)[:C], list(dis)[:B * n])


class Environment:
    """committee.rs:24-28 / :72-83 — threshold, nr_members and the Pedersen commitment key h."""

    def __init__(self, backend: Backend, threshold: int, nr_members: int, ck_gen_bytes: bytes = CK_DEFAULT):
        env_check(threshold, nr_members)
        self.threshold = threshold
        self.nr_members = nr_members
        self.commitment_key = backend.env_init(threshold, nr_members, ck_gen_bytes)
