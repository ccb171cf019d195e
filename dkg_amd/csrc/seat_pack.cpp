// dkg_seat_pack: how the seats (ceremony c, party j) of one operator share the waves of k_seat_horner
// (receivers.hip), and the descriptors the runtime uploads for it.  Every polynomial of a seat is
// evaluated at x = j + 1, so seats with equal x may sit side by side in one wave and keep the
// multiplier wave-uniform.  Host only, a pure function of (n, js); the runtime executes exactly this.
#include <algorithm>
#include <numeric>

#include "../../include/dkg_amd.h"
#include "host_crypto.h"

extern "C" int dkg_seat_pack(size_t n, size_t S, const uint32_t* js, uint32_t* width, uint32_t* per_wave,
                             uint32_t* tiles, uint32_t* wave_of, uint32_t* slot_of, uint32_t* waves) {
  if (n == 0 || (n + 63) / 64 > 0xffffffffu) return DKG_E_ARG;
  uint32_t W = 64;
  if (n < 64)
    for (W = 1; W < n; W *= 2) {}
  const uint32_t per = 64 / W, T = (uint32_t)((n + 63) / 64);
  if (width) *width = W;
  if (per_wave) *per_wave = per;
  if (tiles) *tiles = T;
  if (S == 0) {
    if (waves) *waves = 0;
    return DKG_OK;
  }
  if (!js || !width || !per_wave || !tiles || !wave_of || !slot_of || !waves) return DKG_E_ARG;
  for (size_t p = 0; p < S; p++)
    if (js[p] >= n) return DKG_E_ARG;
  // groups of equal x in ascending order, caller order inside a group
  std::vector<size_t> order(S);
  std::iota(order.begin(), order.end(), (size_t)0);
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return js[a] < js[b]; });
  uint64_t next = 0;  // first wave of the group being filled
  for (size_t g0 = 0; g0 < S;) {
    size_t g1 = g0;
    while (g1 < S && js[order[g1]] == js[order[g0]]) g1++;
    const uint64_t gw = (uint64_t)((g1 - g0 + per - 1) / per) * T;
    if (next + gw > 0xffffffffu) return DKG_E_ARG;
    for (size_t r = 0; r < g1 - g0; r++) {
      wave_of[order[g0 + r]] = (uint32_t)(next + (uint64_t)(r / per) * T);
      slot_of[order[g0 + r]] = (uint32_t)(r % per);
    }
    next += gw;
    g0 = g1;
  }
  *waves = (uint32_t)next;
  return DKG_OK;
}

// The outcome of Phases<Phase5>::finalise for one seat (committee.rs:726-805) from what the seat holds:
// pure host code, the rule dkg_finalise_seats executes for every seat.
extern "C" int dkg_seat_finalise_status(size_t n, size_t t, size_t p, const uint8_t* qualified,
                                        const uint8_t* reconstruct, const uint8_t* a_present, const uint32_t* points,
                                        int r2_error, int r4_error, int32_t* recovery_index) {
  if (recovery_index) *recovery_index = -1;
  if (!n || p >= n || !qualified || !reconstruct || !points) return DKG_E_ARG;
  size_t nq = 0, nr = 0;
  for (size_t i = 0; i < n; i++) {
    if (reconstruct[i] && !qualified[i]) return DKG_E_ARG;  // :746-747 panics
    nq += qualified[i] != 0;
    nr += reconstruct[i] != 0;
  }
  if (r2_error) return DKG_FIN_R2_ERROR;          // :340-347
  if (r4_error) return DKG_FIN_R4_ERROR;          // :567-569
  if (nq - nr <= t) return DKG_FIN_PHASE4_ERROR;  // :673-677
  for (size_t i = 0; i < n; i++) {                // index order, the first failure wins (:745-797)
    int status = DKG_FIN_OK;
    if (reconstruct[i]) {
      if (points[i] < t) status = DKG_FIN_INSUFFICIENT;  // :779-781 (threshold, not t + 1)
    } else if (!qualified[i]) {
      if (i != p) status = DKG_FIN_PANIC;  // :791-794; a disqualified seat adds its own A_p0 (:190)
    } else if (a_present && !a_present[i]) {
      status = DKG_FIN_PANIC;  // never stored (:527-530), as dkg_ceremony_verify_fetched_proven
    }
    if (status != DKG_FIN_OK) {
      if (recovery_index) *recovery_index = (int32_t)i;
      return status;
    }
  }
  return DKG_FIN_OK;
}

namespace dkgh {

int seat_plan(size_t B, size_t n, size_t S, const uint32_t* cer, const uint32_t* js, SeatPlan& out) {
  out = SeatPlan();
  if ((S && !cer) || S >= SEAT_NONE) return DKG_E_ARG;
  for (size_t p = 0; p < S; p++)
    if (cer[p] >= B) return DKG_E_ARG;
  std::vector<uint32_t> wave_of(S), slot_of(S);
  const int rc = dkg_seat_pack(n, S, js, &out.width, &out.per_wave, &out.tiles, wave_of.data(), slot_of.data(), &out.waves);
  if (rc != DKG_OK) return rc;
  distinct_places(S, cer, out.cers, out.seat_col);
  out.seat_x.resize(S);
  out.wave_desc.assign(2 * (size_t)out.waves, 0);
  out.wave_seat.assign((size_t)out.waves * out.per_wave, SEAT_NONE);
  const uint32_t wshift = (uint32_t)seat_wshift(out.width);  // dkg_seat_pack's widths are valid
  for (size_t p = 0; p < S; p++) {
    out.seat_x[p] = js[p] + 1;
    for (uint32_t tile = 0; tile < out.tiles; tile++) {
      const size_t wv = (size_t)wave_of[p] + tile;
      out.wave_desc[2 * wv] = js[p] + 1;
      out.wave_desc[2 * wv + 1] = tile;
      out.wave_seat[seat_cell(wshift, wv, slot_of[p] << wshift)] = (uint32_t)p;  // where the slot's lanes read
    }
  }
  out.live_lanes = S * n;
  return DKG_OK;
}

}  // namespace dkgh
