"""dkg_amd — MI355X-native (gfx950 HIP) backend for the share-generation / share-verification hot
path of the danielSanchezQ/dkg Pedersen-VSS DKG over Ristretto255.  See DESIGN.md."""
from ._lib import (ACCEPT, COMPLAINT_IGNORED, COMPLAINT_NO_PHASE3, COMPLAINT_NOT_OWNED, DKG_PS_NO_COMMITMENT,  # noqa: F401
                   DKG_PS_NO_DISCLOSURE, DKG_PS_OK, MISSING, REJECT, SELF, SKIPPED, DkgError, lib)
from .api import (Backend, BatchProvenResult, BatchResult, MultiBackend, CeremonyResult, ProvenResult, Environment, ceremony_batch_device,  # noqa: F401
                  ceremony_batch_full_device, ceremony_batch_verify, ceremony_batch_verify_full, ceremony_batch_verify_full_proven,
                  ceremony_batch_verify_proven, comb_geometry, dealer_coefficients, enc_randomness, env_check, key_comb_choice, merge_verdicts,
                  packed_row_words, pair_eval_shape, public_share_status, receiver_plan, receiver_plan_constants, seat_disclosures, seat_enc_digits, seat_eval_shape, seat_finalise_status, seat_pack,
                  shard_range, shard_rows, split_multipliers)

__all__ = ["Backend", "MultiBackend", "Environment", "CeremonyResult", "BatchResult", "DkgError", "dealer_coefficients", "env_check",
           "ceremony_batch_device", "ceremony_batch_verify", "ceremony_batch_full_device", "ceremony_batch_verify_full", "enc_randomness", "split_multipliers", "lib",
           "shard_range", "shard_rows", "packed_row_words", "key_comb_choice",
           "ceremony_batch_verify_proven", "ceremony_batch_verify_full_proven", "BatchProvenResult",
           "ACCEPT", "REJECT", "SELF", "SKIPPED", "MISSING", "ProvenResult", "COMPLAINT_IGNORED", "COMPLAINT_NO_PHASE3",
           "COMPLAINT_NOT_OWNED", "merge_verdicts", "receiver_plan", "receiver_plan_constants", "pair_eval_shape",
           "comb_geometry", "seat_pack", "seat_finalise_status", "seat_disclosures", "seat_enc_digits", "seat_eval_shape",
           "public_share_status", "DKG_PS_OK", "DKG_PS_NO_COMMITMENT", "DKG_PS_NO_DISCLOSURE"]
