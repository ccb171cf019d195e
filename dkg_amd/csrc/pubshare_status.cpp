// dkg_public_share_status: whether the public share g s_j of party j follows from one ceremony's public
// data -- the round-3 commitments of the dealers the sum uses and, for every reconstructed dealer, the
// share party j disclosed in phase 5 (BroadcastPhase5, committee.rs:660-669).  Host only, a pure
// function; dkg_public_shares reports exactly this per (ceremony, index).
#include <unordered_set>
#include <vector>

#include "../../include/dkg_amd.h"

extern "C" int dkg_public_share_status(size_t n, const uint8_t* qualified, const uint8_t* reconstruct,
                                       const uint8_t* a_present, uint32_t j, size_t D5, const uint32_t* d_sender,
                                       const uint32_t* d_dealer, int32_t* which) {
  if (which) *which = -1;
  if (!n || j >= n || !qualified || (D5 && (!d_sender || !d_dealer))) return DKG_E_ARG;
  for (size_t i = 0; i < n; i++)
    if (reconstruct && reconstruct[i] && !qualified[i]) return DKG_E_ARG;  // committee.rs:746-747 panics
  std::unordered_set<uint64_t> seen;
  seen.reserve(2 * D5);
  std::vector<uint8_t> have(n, 0);  // dealer i's share disclosed by sender j + 1
  for (size_t d = 0; d < D5; d++) {
    if (d_sender[d] < 1 || d_sender[d] > n || d_dealer[d] < 1 || d_dealer[d] > n) return DKG_E_ARG;
    if (!seen.insert((uint64_t)(d_sender[d] - 1) * n + (d_dealer[d] - 1)).second) return DKG_E_ARG;
    if (d_sender[d] - 1 == j) have[d_dealer[d] - 1] = 1;
  }
  for (size_t i = 0; i < n; i++)  // the sum's own rows first
    if (qualified[i] && !(reconstruct && reconstruct[i]) && a_present && !a_present[i]) {
      if (which) *which = (int32_t)i;
      return DKG_PS_NO_COMMITMENT;
    }
  for (size_t i = 0; i < n; i++)
    if (reconstruct && reconstruct[i] && !have[i]) {
      if (which) *which = (int32_t)i;
      return DKG_PS_NO_DISCLOSURE;
    }
  return DKG_PS_OK;
}
