"""ctypes binding of the in-tree HIP library dkg_amd/libdkg_amd.so (C ABI: include/dkg_amd.h).

The product path always runs the HIP kernels: there is no CPU fallback.  If the library is missing
or no GPU is visible, the calls below raise instead of silently computing something else.
"""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DKG_AMD_LIB", os.path.join(HERE, "libdkg_amd.so"))

DKG_OK = 0
DKG_E_ARG = -1
DKG_E_DECODE = -2
DKG_E_DEVICE = -3
DKG_E_NOMEM = -4
REJECT, ACCEPT, SELF, SKIPPED, MISSING = 0, 1, 2, 3, 4
# per-party finalise status (dkg_finalise_parties)
FIN_OK, FIN_R2_ERROR, FIN_R4_ERROR, FIN_PHASE4_ERROR, FIN_INSUFFICIENT, FIN_PANIC = 0, 1, 2, 3, 4, 5
# complaint verdicts beyond the primitives' 0..3 and -1 (dkg_complaints_verify, dkg_complaints3_verify)
COMPLAINT_IGNORED, COMPLAINT_NO_PHASE3 = 4, 5
# a sharded proven call's verdict for a complaint against another rank's dealer: below every real code, so
# that the element-wise maximum over the ranks' arrays is the ceremony's verdict list
COMPLAINT_NOT_OWNED = -2
# dkg_public_shares / dkg_public_share_status
DKG_PS_OK, DKG_PS_NO_COMMITMENT, DKG_PS_NO_DISCLOSURE = 0, 1, 2

_lib = None


class DkgError(RuntimeError):
    def __init__(self, code, msg=""):
        self.code = code
        names = {DKG_E_ARG: "DKG_E_ARG", DKG_E_DECODE: "DKG_E_DECODE", DKG_E_DEVICE: "DKG_E_DEVICE",
                 DKG_E_NOMEM: "DKG_E_NOMEM"}
        super().__init__(f"{names.get(code, code)}: {msg}")


class CeremonyOut(ctypes.Structure):
    _fields_ = [
        ("E", ctypes.c_void_p), ("A", ctypes.c_void_p),
        ("s", ctypes.c_void_p), ("s_prime", ctypes.c_void_p),
        ("dec2", ctypes.c_void_p), ("dec4", ctypes.c_void_p),
        ("qualified", ctypes.c_void_p), ("r2_error", ctypes.c_void_p), ("r4_error", ctypes.c_void_p),
        ("complaints2", ctypes.c_void_p), ("reconstruct", ctypes.c_void_p),
        ("final_share", ctypes.c_void_p), ("public_share", ctypes.c_void_p),
        ("mpk", ctypes.c_uint8 * 32),
        ("n_qualified", ctypes.c_int32), ("phase4_error", ctypes.c_int32),
        ("ms_round1", ctypes.c_double), ("ms_round2", ctypes.c_double), ("ms_round3", ctypes.c_double),
        ("ms_round4", ctypes.c_double), ("ms_finalise", ctypes.c_double), ("ms_total", ctypes.c_double),
    ]


class ReceiverPlan(ctypes.Structure):
    """dkg_receiver_plan (include/dkg_amd.h)."""
    _fields_ = [("chunk", ctypes.c_uint32), ("stages", ctypes.c_uint32), ("arity", ctypes.c_uint32 * 16),
                ("mult", (ctypes.c_uint8 * 32) * 16)]


class ShardOutcome(ctypes.Structure):
    _fields_ = [
        ("qualified", ctypes.c_void_p), ("complaints2", ctypes.c_void_p), ("r2_error", ctypes.c_void_p),
        ("reconstruct", ctypes.c_void_p), ("r4_error", ctypes.c_void_p),
        ("n_qualified", ctypes.c_int32), ("phase4_error", ctypes.c_int32),
    ]


class BatchOut(ctypes.Structure):
    _fields_ = [
        ("mpk", ctypes.c_void_p), ("n_qualified", ctypes.c_void_p), ("phase4_error", ctypes.c_void_p),
        ("qualified", ctypes.c_void_p),
        ("r2_error", ctypes.c_void_p), ("r4_error", ctypes.c_void_p), ("complaints2", ctypes.c_void_p),
        ("reconstruct", ctypes.c_void_p), ("final_share", ctypes.c_void_p), ("public_share", ctypes.c_void_p),
        ("dec2", ctypes.c_void_p), ("dec4", ctypes.c_void_p),
        ("ms_round1", ctypes.c_double), ("ms_checks", ctypes.c_double), ("ms_round3", ctypes.c_double),
        ("ms_finalise", ctypes.c_double), ("ms_total", ctypes.c_double),
    ]


def lib():
    """Load libdkg_amd.so (raises if it is absent: the HIP path is mandatory)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -C dkg_amd` or __graft_entry__.build()")
    # When torch shares the process, its HIP runtime must be the one the dynamic loader binds
    # first: loading libdkg_amd.so (linked against /opt/rocm's libamdhip64) before torch leaves
    # torch.cuda without a device.  Import torch first whenever it is importable; a torch install
    # that fails to import for any reason (its ROCm libraries included) must not stop the library
    # from loading for callers that never use torch (DKG_NO_TORCH_PREIMPORT=1 skips the attempt).
    if "torch" not in sys.modules and not os.environ.get("DKG_NO_TORCH_PREIMPORT"):
        try:
            import torch  # noqa: F401
        except Exception:  # noqa: BLE001 -- ImportError, OSError, RuntimeError from a broken install
            pass
    L = ctypes.CDLL(LIB_PATH)
    sz, p, u8p = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_char_p
    L.dkg_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(p)]
    L.dkg_ctx_destroy.argtypes = [p]
    L.dkg_ctx_destroy.restype = None
    L.dkg_ctx_last_error.argtypes = [p]
    L.dkg_ctx_last_error.restype = ctypes.c_char_p
    L.dkg_device_count.argtypes = []
    L.dkg_ctx_set_streams.argtypes = [p, ctypes.c_int]
    L.dkg_ctx_set_overlap.argtypes = [p, ctypes.c_int]
    L.dkg_ctx_set_verify_mode.argtypes = [p, ctypes.c_int]
    L.dkg_ctx_fallback_rows.argtypes = [p]
    L.dkg_ctx_fallback_rows.restype = sz
    L.dkg_ctx_set_split.argtypes = [p, ctypes.c_int]
    L.dkg_ctx_set_stepping.argtypes = [p, ctypes.c_int]
    L.dkg_ctx_set_field_mode.argtypes = [p, ctypes.c_int]
    L.dkg_ctx_set_binomial.argtypes = [p, ctypes.c_int]
    L.dkg_ctx_set_check.argtypes = [p, ctypes.c_int]
    L.dkg_ctx_last_split.argtypes = [p]
    L.dkg_ctx_last_split_len.argtypes = [p]
    L.dkg_ctx_last_split_len.restype = sz
    L.dkg_split_model_ms.argtypes = [sz, sz, sz, ctypes.c_int]
    L.dkg_split_model_ms.restype = ctypes.c_double
    L.dkg_split_len.argtypes = [sz, sz, sz, ctypes.c_int]
    L.dkg_split_len.restype = sz
    L.dkg_ctx_set_combine.argtypes = [p, ctypes.c_int]
    L.dkg_ctx_last_combine.argtypes = [p]
    L.dkg_ctx_last_binomial.argtypes = [p]
    L.dkg_ctx_set_addends.argtypes = [p, ctypes.c_int]
    L.dkg_ctx_set_stepping_formula.argtypes = [p, ctypes.c_int]
    L.dkg_ctx_stepping_redos.argtypes = [p]
    L.dkg_ctx_stepping_redos.restype = ctypes.c_longlong
    L.dkg_ctx_binomial_reruns.argtypes = [p]
    L.dkg_ctx_binomial_wave_redos.argtypes = [p]
    L.dkg_ctx_binomial_wave_redos.restype = ctypes.c_longlong
    L.dkg_ctx_clock_probe.argtypes = [p, ctypes.c_uint, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    L.dkg_device_pci_bus_id.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    L.dkg_split_multipliers.argtypes = [sz, sz, ctypes.c_int, p, p]
    if hasattr(L, "dkg_zero_tests"):  # a test aid: absent from an older library loaded through DKG_AMD_LIB
        L.dkg_zero_tests.argtypes = [p, sz, p, p]
    if hasattr(L, "dkg_fe_ops"):  # test aids, likewise
        L.dkg_fe_ops.argtypes = [p, ctypes.c_int, ctypes.c_int, sz, p, p]
    if hasattr(L, "dkg_sc_ops"):
        L.dkg_sc_ops.argtypes = [p, ctypes.c_int, sz, p, p]
    L.dkg_jsf_digits.argtypes = [p, p, p, p, p]
    L.dkg_split_digits.argtypes = [sz, sz, ctypes.c_int, ctypes.c_int, p, p]
    L.dkg_ctx_phase_ms.argtypes = [p, ctypes.c_char_p]
    L.dkg_ctx_phase_ms.restype = ctypes.c_double
    L.dkg_env_check.argtypes = [sz, sz]
    L.dkg_env_init.argtypes = [p, sz, sz, u8p, sz, p]
    L.dkg_msm_batch.argtypes = [p, sz, sz, u8p, u8p, p]
    L.dkg_fixed_base_batch.argtypes = [p, p, sz, u8p, p]
    L.dkg_poly_eval_batch.argtypes = [p, sz, sz, u8p, sz, p, p]
    L.dkg_points_valid_batch.argtypes = [p, sz, u8p, p]
    L.dkg_share_gen.argtypes = [p, sz, sz, sz, u8p, u8p, p, p, p, p]
    L.dkg_verify_pairs.argtypes = [p, sz, sz, ctypes.c_int, sz, sz, u8p, u8p, p, p]
    L.dkg_verify_receiver.argtypes = [p, sz, sz, ctypes.c_int, sz, u8p, u8p, p, p]
    L.dkg_receiver_plan_for.argtypes = [sz, sz, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(ReceiverPlan)]
    L.dkg_receiver_plan_cost_us.argtypes = [sz, sz, ctypes.c_uint32, ctypes.POINTER(ReceiverPlan)]
    L.dkg_receiver_plan_cost_us.restype = ctypes.c_double
    L.dkg_receiver_plan_constants.argtypes = [ctypes.POINTER(ctypes.c_double)]
    L.dkg_receiver_plan_constants.restype = None
    L.dkg_ctx_set_receiver_chunk.argtypes = [p, ctypes.c_int]
    L.dkg_ctx_last_receiver_chunk.argtypes = [p]
    L.dkg_commitment_eval.argtypes = [p, sz, sz, sz, p, u8p, p, p]
    if hasattr(L, "dkg_pair_eval_shape"):  # absent from an older library loaded through DKG_AMD_LIB
        L.dkg_pair_eval_shape.argtypes = [sz, ctypes.c_int] + [ctypes.POINTER(ctypes.c_uint32)] * 3
        L.dkg_commitment_eval_pairs.argtypes = [p, sz, sz, sz, p, p, u8p, p, p]
    L.dkg_verify_receivers.argtypes = [p, sz, sz, ctypes.c_int, sz, p, u8p, u8p, p, p, p]
    L.dkg_party_round2.argtypes = [p, sz, sz, sz, u8p, u8p, u8p, u8p, p, p, p, p, p, p, p]
    if hasattr(L, "dkg_seat_pack"):  # absent from an older library loaded through DKG_AMD_LIB
        L.dkg_seat_pack.argtypes = [sz, sz, p] + [ctypes.POINTER(ctypes.c_uint32)] * 3 + [p, p, ctypes.POINTER(ctypes.c_uint32)]
        L.dkg_commitment_eval_seats.argtypes = [p, sz, sz, sz, sz, p, p, u8p, p, p]
        L.dkg_verify_seats.argtypes = [p, sz, sz, sz, ctypes.c_int, sz, p, p, u8p, u8p, p, p, p]
        L.dkg_party_round2_seats.argtypes = [p, sz, sz, sz, sz, p, p, u8p, u8p, u8p, u8p, p, p, p, p, p, p, p]
    if hasattr(L, "dkg_finalise_seats"):  # absent from an older library loaded through DKG_AMD_LIB
        L.dkg_complaints_verify_ceremonies.argtypes = [p, sz, sz, sz, sz, p, p, p, u8p, u8p, u8p, u8p, u8p, p, p]
        L.dkg_complaints3_verify_ceremonies.argtypes = [p, sz, sz, sz, sz, p, p, p, u8p, u8p, u8p, u8p, u8p, u8p, p, p]
        L.dkg_party_round3_seats.argtypes = [p, sz, sz, sz, sz, p, p, u8p, u8p, p, p]
        L.dkg_finalise_seats.argtypes = [p, sz, sz, sz, sz, p, p, u8p, u8p, u8p, u8p, u8p, u8p, u8p, sz, p, p, p, u8p,
                                         p, p, p]
        L.dkg_seat_finalise_status.argtypes = [sz, sz, sz, u8p, u8p, u8p, p, ctypes.c_int, ctypes.c_int, p]
    if hasattr(L, "dkg_party_round1_seats"):  # absent from an older library loaded through DKG_AMD_LIB
        L.dkg_party_round1_seats.argtypes = [p, sz, sz, sz, sz, p, p, u8p, u8p, u8p, u8p, p, p, p, p, p, p, p]
        L.dkg_ctx_set_seat_deal.argtypes = [p, ctypes.c_int]
        L.dkg_ctx_last_seat_deal.argtypes = [p]
        L.dkg_seat_enc_digits.argtypes = [p, p, ctypes.POINTER(ctypes.c_int)]
    if hasattr(L, "dkg_seat_eval_shape"):  # absent from an older library loaded through DKG_AMD_LIB
        L.dkg_seat_eval_shape.argtypes = [sz, sz, sz, ctypes.c_uint32, ctypes.c_int] + [ctypes.POINTER(ctypes.c_uint32)] * 3 + [
            ctypes.POINTER(ctypes.c_uint64)]
        L.dkg_seat_eval_constants.argtypes = [ctypes.POINTER(ctypes.c_double)]
        L.dkg_seat_eval_constants.restype = None
        L.dkg_ctx_set_seat_eval.argtypes = [p, ctypes.c_int, ctypes.c_int]
        L.dkg_ctx_last_seat_eval.argtypes = [p, ctypes.POINTER(ctypes.c_int)]
    if hasattr(L, "dkg_public_shares"):  # absent from an older library loaded through DKG_AMD_LIB
        L.dkg_commitment_sum.argtypes = [p, sz, sz, sz, u8p, u8p, p, p]
        L.dkg_public_shares.argtypes = [p, sz, sz, sz, u8p, u8p, u8p, u8p, sz, p, sz, p, p, p, u8p, p, p, p, p]
        L.dkg_public_share_status.argtypes = [sz, u8p, u8p, u8p, ctypes.c_uint32, sz, p, p, p]
        L.dkg_ctx_set_public_share_slab.argtypes = [p, sz]
    L.dkg_ceremony_run.argtypes = [p, sz, sz, u8p, u8p, ctypes.POINTER(CeremonyOut)]
    L.dkg_ceremony_verify.argtypes = [p, sz, sz, u8p, u8p, u8p, u8p, ctypes.POINTER(CeremonyOut)]
    L.dkg_ceremony_verify_fetched.argtypes = [p, sz, sz, u8p, u8p, u8p, u8p, u8p, u8p, ctypes.POINTER(CeremonyOut)]
    L.dkg_ceremony_run_device.argtypes = [p, sz, sz, p, p, ctypes.POINTER(CeremonyOut)]
    L.dkg_ceremony_shard_device.argtypes = [p, sz, sz, sz, sz, p, p, p, p, p, p, ctypes.POINTER(ctypes.c_double)]
    L.dkg_ceremony_shard_verify_device.argtypes = [p, sz, sz, sz, sz, p, p, p, p, p, p, p, p,
                                                    ctypes.POINTER(ctypes.c_double)]
    L.dkg_ceremony_shard_full_device.argtypes = [p, sz, sz, sz, sz, p, p, p, u8p, u8p, p, p, p, p, p, p,
                                                  ctypes.POINTER(ctypes.c_double)]
    L.dkg_ceremony_shard_verify_full_device.argtypes = [p, sz, sz, sz, sz, p, p, p, p, u8p, p, p, p, p,
                                                         ctypes.POINTER(ctypes.c_double)]
    L.dkg_ctx_set_key_comb.argtypes = [p, ctypes.c_int]
    L.dkg_ctx_last_key_comb.argtypes = [p]
    L.dkg_key_comb_choice.argtypes = [sz, sz, ctypes.c_int, ctypes.c_int]
    L.dkg_key_comb_constants.argtypes = [ctypes.POINTER(ctypes.c_double)]
    L.dkg_key_comb_constants.restype = None
    L.dkg_ceremony_batch_device.argtypes = [p, sz, sz, sz, p, p, ctypes.POINTER(BatchOut)]
    L.dkg_ceremony_batch_verify.argtypes = [p, sz, sz, sz, u8p, u8p, u8p, u8p, ctypes.POINTER(BatchOut)]
    L.dkg_dealer_coeffs_device.argtypes = [p, u8p, ctypes.c_uint32, sz, sz, sz, sz, p, p]
    L.dkg_member_keys.argtypes = [p, u8p, ctypes.c_uint32, sz, p, p]
    L.dkg_enc_randomness.argtypes = [u8p, ctypes.c_uint32, sz, sz, sz, sz, p]
    L.dkg_enc_randomness_device.argtypes = [p, u8p, ctypes.c_uint32, sz, sz, sz, sz, sz, p]
    L.dkg_encrypt_shares.argtypes = [p, sz, sz, u8p, u8p, u8p, u8p, p, p]
    L.dkg_decrypt_shares.argtypes = [p, sz, sz, u8p, u8p, u8p, p, p, p]
    L.dkg_ceremony_run_full_device.argtypes = [p, sz, sz, p, p, p, u8p, u8p, ctypes.POINTER(CeremonyOut)]
    L.dkg_ceremony_verify_full.argtypes = [p, sz, sz, u8p, u8p, u8p, u8p, u8p, ctypes.POINTER(CeremonyOut)]
    L.dkg_member_keys_batch.argtypes = [p, u8p, ctypes.c_uint32, sz, sz, p, p]
    L.dkg_encrypt_shares_batch.argtypes = [p, sz, sz, u8p, u8p, u8p, u8p, p, p]
    L.dkg_decrypt_shares_batch.argtypes = [p, sz, sz, u8p, u8p, u8p, p, p, p]
    L.dkg_ceremony_batch_full_device.argtypes = [p, sz, sz, sz, p, p, p, u8p, u8p, ctypes.POINTER(BatchOut)]
    L.dkg_ceremony_batch_verify_full.argtypes = [p, sz, sz, sz, u8p, u8p, u8p, u8p, u8p, ctypes.POINTER(BatchOut),
                                                 p, p]
    L.dkg_ctx_set_batch_full_chunk.argtypes = [p, sz]
    L.dkg_misbehaviour_prove.argtypes = [p, sz, u8p, u8p, u8p, p]
    L.dkg_complaint1_verify.argtypes = [p, sz, sz, p, u8p, u8p, u8p, u8p, p]
    L.dkg_complaint3_verify.argtypes = [p, sz, sz, p, u8p, u8p, u8p, u8p, p]
    L.dkg_complaints_prove.argtypes = [p, sz, u8p, u8p, u8p, p]
    L.dkg_complaints_verify.argtypes = [p, sz, sz, sz, p, p, u8p, u8p, u8p, u8p, u8p, p, p]
    L.dkg_ctx_set_complaint_eval.argtypes = [p, ctypes.c_int]
    L.dkg_ceremony_verify_full_complaints.argtypes = [p, sz, sz, u8p, u8p, u8p, u8p, u8p, u8p, sz, p, p, u8p,
                                                      ctypes.POINTER(CeremonyOut), p, p]
    L.dkg_complaints3_verify.argtypes = [p, sz, sz, sz, p, p, u8p, u8p, u8p, u8p, u8p, u8p, p, p]
    L.dkg_ceremony_verify_fetched_proven.argtypes = [p, sz, sz, u8p, u8p, u8p, u8p, u8p, u8p, sz, p, p, u8p, u8p,
                                                     ctypes.POINTER(CeremonyOut), p, p, p]
    L.dkg_ceremony_verify_full_proven.argtypes = [p, sz, sz, u8p, u8p, u8p, u8p, u8p, u8p, sz, p, p, u8p, u8p, sz, p, p,
                                                  u8p, u8p, ctypes.POINTER(CeremonyOut), p, p, p, p, p]
    L.dkg_ceremony_batch_verify_proven.argtypes = [p, sz, sz, sz, u8p, u8p, u8p, u8p, u8p, u8p, sz, p, p, p, u8p, u8p,
                                                   ctypes.POINTER(BatchOut), p, p, p]
    L.dkg_ceremony_batch_verify_full_proven.argtypes = [p, sz, sz, sz, u8p, u8p, u8p, u8p, u8p, u8p, sz, p, p, p, u8p,
                                                        u8p, sz, p, p, p, u8p, u8p, ctypes.POINTER(BatchOut), p, p, p, p,
                                                        p, p, p]
    L.dkg_ceremony_shard_verify_proven_device.argtypes = [p, sz, sz, sz, sz, p, p, p, p, u8p, u8p, sz, p, p, u8p, u8p,
                                                           p, p, p, p, sz, p, p, ctypes.POINTER(ctypes.c_double)]
    L.dkg_ceremony_shard_verify_full_proven_device.argtypes = [p, sz, sz, sz, sz, p, p, p, p, u8p, u8p, u8p, u8p, sz, p,
                                                                p, u8p, sz, p, p, u8p, u8p, p, p, p, p, sz, p, p, p, p,
                                                                ctypes.POINTER(ctypes.c_double)]
    L.dkg_ctx_last_complaint_eval.argtypes = [p]
    L.dkg_shard_combine_proven_device.argtypes = [p, sz, sz, sz, p, p, p, p, ctypes.c_int, p, p,
                                                  ctypes.POINTER(ShardOutcome), p, p, p]
    L.dkg_multi_ceremony_verify_proven.argtypes = [p, sz, sz, u8p, u8p, u8p, u8p, u8p, u8p, sz, p, p, u8p, u8p,
                                                   ctypes.POINTER(CeremonyOut), p, p, p]
    L.dkg_multi_ceremony_verify_full_proven.argtypes = [p, sz, sz, u8p, u8p, u8p, u8p, u8p, u8p, sz, p, p, u8p, u8p, sz,
                                                        p, p, u8p, u8p, ctypes.POINTER(CeremonyOut), p, p, p, p, p]
    L.dkg_dealer_coeffs.argtypes = [u8p, ctypes.c_uint32, sz, sz, sz, p, p]
    L.dkg_scalar_sum_device.argtypes = [p, sz, sz, p, p, p]
    L.dkg_point_sum_device.argtypes = [p, sz, p, p, p]
    L.dkg_share_gen_device.argtypes = [p, sz, sz, sz, p, p, p, p, p, p]
    L.dkg_ceremony_shard_recon_device.argtypes = [p, sz, sz, sz, sz, u8p, u8p, u8p, u8p, p, p,
                                                  ctypes.POINTER(ctypes.c_int32)]
    L.dkg_finalise_parties.argtypes = [p, sz, sz, u8p, u8p, u8p, u8p, u8p, u8p, u8p, p, p, p]
    L.dkg_shard_range.argtypes = [sz, sz, sz, ctypes.POINTER(sz), ctypes.POINTER(sz)]
    L.dkg_shard_range.restype = None
    L.dkg_shard_rows.argtypes = [sz, sz]
    L.dkg_shard_rows.restype = sz
    L.dkg_shard_combine_device.argtypes = [p, sz, sz, sz, p, p, p, p, ctypes.POINTER(ShardOutcome)]
    L.dkg_shard_combine_packed_device.argtypes = [p, sz, sz, sz, p, p, p, p, ctypes.POINTER(ShardOutcome)]
    L.dkg_fixed_base_windows.argtypes = []
    L.dkg_key_comb_windows.argtypes = []
    if hasattr(L, "dkg_comb_geometry"):  # absent from an older library loaded through DKG_AMD_LIB
        L.dkg_ctx_set_comb_build.argtypes = [p, ctypes.c_int]
        L.dkg_ctx_last_comb_build.argtypes = [p]
        L.dkg_ctx_last_comb_build_ms.argtypes = [p]
        L.dkg_ctx_last_comb_build_ms.restype = ctypes.c_double
        L.dkg_comb_geometry.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                        ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
        L.dkg_comb_entries.argtypes = [p, ctypes.c_int, u8p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, p]
    L.dkg_packed_row_words.argtypes = [sz]
    L.dkg_packed_row_words.restype = sz
    L.dkg_decisions_pack_device.argtypes = [p, sz, sz, sz, sz, p, p]
    L.dkg_shard_finalise_device.argtypes = [p, sz, sz, sz, p, p, u8p, ctypes.c_int, p, p, p]
    L.dkg_multi_create.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(p)]
    L.dkg_multi_destroy.argtypes = [p]
    L.dkg_multi_destroy.restype = None
    L.dkg_multi_size.argtypes = [p]
    L.dkg_multi_ctx.argtypes = [p, ctypes.c_int]
    L.dkg_multi_ctx.restype = p
    L.dkg_multi_last_error.argtypes = [p]
    L.dkg_multi_last_error.restype = ctypes.c_char_p
    L.dkg_multi_phase_ms.argtypes = [p, ctypes.c_char_p]
    L.dkg_multi_phase_ms.restype = ctypes.c_double
    L.dkg_multi_env_init.argtypes = [p, sz, sz, u8p, sz, p]
    L.dkg_multi_ceremony_run.argtypes = [p, sz, sz, u8p, u8p, ctypes.POINTER(CeremonyOut)]
    L.dkg_multi_ceremony_run_device.argtypes = [p, sz, sz, ctypes.POINTER(p), ctypes.POINTER(p),
                                                ctypes.POINTER(CeremonyOut)]
    L.dkg_multi_ceremony_verify.argtypes = [p, sz, sz, u8p, u8p, u8p, u8p, ctypes.POINTER(CeremonyOut)]
    L.dkg_multi_ceremony_run_full.argtypes = [p, sz, sz, u8p, u8p, u8p, u8p, u8p, ctypes.POINTER(CeremonyOut)]
    L.dkg_multi_ceremony_run_full_device.argtypes = [p, sz, sz, ctypes.POINTER(p), ctypes.POINTER(p), ctypes.POINTER(p),
                                                     u8p, u8p, ctypes.POINTER(CeremonyOut)]
    L.dkg_multi_ceremony_verify_full.argtypes = [p, sz, sz, u8p, u8p, u8p, u8p, u8p, ctypes.POINTER(CeremonyOut)]
    _lib = L
    return L


EXPORTED = [
    "dkg_ctx_create", "dkg_ctx_destroy", "dkg_ctx_last_error", "dkg_ctx_phase_ms", "dkg_ctx_set_streams", "dkg_ctx_set_overlap",
    "dkg_device_count", "dkg_env_init",
    "dkg_env_check", "dkg_msm_batch", "dkg_fixed_base_batch", "dkg_poly_eval_batch",
    "dkg_points_valid_batch", "dkg_share_gen", "dkg_verify_pairs", "dkg_verify_receiver",
    "dkg_ctx_set_split", "dkg_ctx_set_stepping", "dkg_ctx_set_field_mode", "dkg_ctx_set_binomial", "dkg_ctx_set_check", "dkg_ctx_last_split", "dkg_ctx_last_split_len", "dkg_ctx_set_verify_mode", "dkg_ctx_fallback_rows", "dkg_split_model_ms", "dkg_split_len",
    "dkg_ctx_set_combine", "dkg_ctx_last_combine", "dkg_ctx_last_binomial", "dkg_ctx_set_addends", "dkg_ctx_set_stepping_formula", "dkg_ctx_stepping_redos", "dkg_zero_tests", "dkg_fe_ops", "dkg_sc_ops", "dkg_stepping_lane_map", "dkg_ctx_binomial_reruns", "dkg_ctx_binomial_wave_redos", "dkg_split_multipliers", "dkg_jsf_digits", "dkg_split_digits",
    "dkg_ctx_clock_probe", "dkg_device_pci_bus_id",
    "dkg_ceremony_run", "dkg_ceremony_verify", "dkg_ceremony_verify_fetched", "dkg_ceremony_run_device", "dkg_ceremony_shard_device",
    "dkg_ceremony_shard_verify_device",
    "dkg_ceremony_batch_device", "dkg_ceremony_batch_verify", "dkg_member_keys", "dkg_enc_randomness",
    "dkg_enc_randomness_device", "dkg_encrypt_shares", "dkg_decrypt_shares", "dkg_ceremony_run_full_device",
    "dkg_ceremony_verify_full", "dkg_misbehaviour_prove", "dkg_complaint1_verify", "dkg_complaint3_verify", "dkg_dealer_coeffs", "dkg_dealer_coeffs_device",
    "dkg_scalar_sum_device", "dkg_point_sum_device", "dkg_ceremony_shard_recon_device", "dkg_finalise_parties",
    "dkg_share_gen_device", "dkg_shard_range", "dkg_shard_rows", "dkg_shard_combine_device",
    "dkg_shard_combine_packed_device", "dkg_packed_row_words", "dkg_fixed_base_windows", "dkg_key_comb_windows", "dkg_decisions_pack_device",
    "dkg_shard_finalise_device", "dkg_multi_create", "dkg_multi_destroy", "dkg_multi_size", "dkg_multi_ctx",
    "dkg_multi_last_error", "dkg_multi_phase_ms", "dkg_multi_env_init", "dkg_multi_ceremony_run",
    "dkg_multi_ceremony_run_device", "dkg_multi_ceremony_verify",
    "dkg_member_keys_batch", "dkg_encrypt_shares_batch", "dkg_decrypt_shares_batch", "dkg_ceremony_batch_full_device",
    "dkg_ceremony_batch_verify_full", "dkg_ctx_set_batch_full_chunk",
    "dkg_complaints_prove", "dkg_complaints_verify", "dkg_ctx_set_complaint_eval", "dkg_ceremony_verify_full_complaints",
    "dkg_complaints3_verify", "dkg_ceremony_verify_fetched_proven", "dkg_ceremony_verify_full_proven",
    "dkg_ceremony_batch_verify_proven", "dkg_ceremony_batch_verify_full_proven",
    "dkg_ceremony_shard_full_device", "dkg_ceremony_shard_verify_full_device", "dkg_ctx_set_key_comb",
    "dkg_ctx_last_key_comb", "dkg_key_comb_choice", "dkg_key_comb_constants", "dkg_multi_ceremony_run_full",
    "dkg_multi_ceremony_run_full_device", "dkg_multi_ceremony_verify_full",
    "dkg_ceremony_shard_verify_proven_device", "dkg_ceremony_shard_verify_full_proven_device",
    "dkg_ctx_last_complaint_eval", "dkg_shard_combine_proven_device",
    "dkg_multi_ceremony_verify_proven", "dkg_multi_ceremony_verify_full_proven",
    "dkg_receiver_plan_for", "dkg_receiver_plan_cost_us", "dkg_receiver_plan_constants", "dkg_ctx_set_receiver_chunk",
    "dkg_ctx_set_comb_build", "dkg_ctx_last_comb_build", "dkg_ctx_last_comb_build_ms", "dkg_comb_geometry", "dkg_comb_entries",
    "dkg_ctx_last_receiver_chunk", "dkg_pair_eval_shape", "dkg_commitment_eval_pairs", "dkg_commitment_eval", "dkg_verify_receivers", "dkg_party_round2",
    "dkg_seat_pack", "dkg_commitment_eval_seats", "dkg_verify_seats", "dkg_party_round2_seats",
    "dkg_complaints_verify_ceremonies", "dkg_complaints3_verify_ceremonies", "dkg_party_round3_seats", "dkg_finalise_seats",
    "dkg_seat_finalise_status",
    "dkg_party_round1_seats", "dkg_ctx_set_seat_deal", "dkg_ctx_last_seat_deal", "dkg_seat_enc_digits",
    "dkg_seat_eval_shape", "dkg_seat_eval_constants", "dkg_ctx_set_seat_eval", "dkg_ctx_last_seat_eval",
    "dkg_commitment_sum", "dkg_public_shares", "dkg_public_share_status", "dkg_ctx_set_public_share_slab",
]
