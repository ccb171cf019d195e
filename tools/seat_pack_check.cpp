// Stand-alone host check of the seats calls' plain C++: dkg_seat_pack and the descriptor builder
// (dkgh::seat_plan: distinct ceremonies, per-wave and per-seat records), read lane by lane through
// seat_map.h, the lane map k_seat_horner itself runs.  Meant to be built with -fsanitize=address,undefined
// and run on the CPU:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/seat_pack_check.cpp dkg_amd/csrc/seat_pack.cpp dkg_amd/csrc/receiver_plan.cpp \
//       dkg_amd/csrc/host_crypto.cpp -o seat_pack_check
// Exit status 0 and "ok" when every check holds.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "../dkg_amd/csrc/host_crypto.h"
#include "../include/dkg_amd.h"

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "%s:%d: %s fails\n", __FILE__, __LINE__, #c); \
      return 1;                                                    \
    }                                                              \
  } while (0)

static uint32_t seed = 2463534242u;
static uint32_t rnd() {
  seed = seed * 1664525u + 1013904223u;
  return seed >> 8;
}

// one seat list through dkg_seat_pack and seat_plan; the kernel's reads (seat_map.h) with bounds
static int run(size_t B, size_t n, const std::vector<uint32_t>& cer, const std::vector<uint32_t>& js) {
  const size_t S = js.size();
  uint32_t W = 0, per = 0, tiles = 0, waves = 0;
  std::vector<uint32_t> wave_of(S), slot_of(S);
  CHECK(dkg_seat_pack(n, S, js.data(), &W, &per, &tiles, wave_of.data(), slot_of.data(), &waves) == DKG_OK);
  CHECK(W >= 1 && W <= 64 && (W & (W - 1)) == 0 && per == 64 / W && tiles == (n + 63) / 64);
  CHECK(n >= 64 ? W == 64 : (W >= n && W < 2 * n));
  std::map<uint32_t, size_t> count;
  for (uint32_t j : js) count[j]++;
  size_t want = 0;
  for (auto& kv : count) want += (kv.second + per - 1) / per * tiles;
  CHECK(waves == want);

  dkgh::SeatPlan pl;
  CHECK(dkgh::seat_plan(B, n, S, cer.data(), js.data(), pl) == DKG_OK);
  CHECK(pl.width == W && pl.per_wave == per && pl.tiles == tiles && pl.waves == waves);
  CHECK(pl.seat_col.size() == S && pl.seat_x.size() == S && pl.wave_desc.size() == 2 * (size_t)waves &&
        pl.wave_seat.size() == (size_t)waves * per && pl.live_lanes == S * n);
  for (size_t p = 0; p < S; p++)
    CHECK(pl.seat_col[p] < pl.cers.size() && pl.cers[pl.seat_col[p]] == cer[p] && pl.seat_x[p] == js[p] + 1);
  for (size_t a = 0; a < pl.cers.size(); a++)
    for (size_t b = a + 1; b < pl.cers.size(); b++) CHECK(pl.cers[a] != pl.cers[b]);
  // the kernel's view: wave v, lane l -> (seat, dealer) or dead; every pair exactly once
  const size_t cols = (pl.cers.size() * n + 63) / 64 * 64;
  std::vector<uint8_t> seen(S * n, 0);
  const uint32_t wshift = (uint32_t)seat_wshift(W);  // W is a valid width: checked above
  for (size_t v = 0; v < waves; v++) {
    const uint32_t x = pl.wave_desc[2 * v], tile = pl.wave_desc[2 * v + 1];
    CHECK(x >= 1 && x <= n && tile < tiles);
    CHECK(v == 0 || pl.wave_desc[2 * (v - 1)] <= x);  // groups in ascending x
    bool any = false;
    for (uint32_t l = 0; l < 64; l++) {
      CHECK(seat_cell(wshift, v, l) < pl.wave_seat.size());
      const SeatLane m = seat_lane(n, wshift, v, l, pl.wave_desc.data(), pl.wave_seat.data());
      if (!m.live) continue;
      const uint32_t seat = m.seat;
      CHECK(seat < S && js[seat] + 1 == x);
      CHECK(wave_of[seat] + tile == v && slot_of[seat] == m.slot);
      CHECK(seat_column(m, n, pl.seat_col.data()) < cols);
      CHECK(!seen[seat_result(m, n)]);
      seen[seat_result(m, n)] = 1;
      any = true;
    }
    CHECK(any);  // no wave without a live lane
  }
  for (uint8_t s : seen) CHECK(s);
  return 0;
}

int main() {
  for (size_t n : {(size_t)1, (size_t)2, (size_t)3, (size_t)10, (size_t)16, (size_t)32, (size_t)33, (size_t)64,
                   (size_t)70, (size_t)130, (size_t)1000})
    for (size_t S : {(size_t)1, (size_t)2, (size_t)63, (size_t)64, (size_t)65, (size_t)1000, (size_t)5000}) {
      const size_t B = S / 2 + 1;
      std::vector<uint32_t> cer(S), js(S);
      for (int shape = 0; shape < 3; shape++) {
        for (size_t p = 0; p < S; p++) {
          cer[p] = rnd() % (uint32_t)B;
          js[p] = shape == 0 ? rnd() % (uint32_t)n : shape == 1 ? (uint32_t)(n - 1) : rnd() % (uint32_t)(n < 3 ? n : 3);
        }
        if (run(B, n, cer, js)) return 1;
      }
    }
  // arguments
  uint32_t v[4], js3[3] = {0, 1, 2}, cer3[3] = {0, 1, 5}, wo[3], so[3];
  CHECK(dkg_seat_pack(0, 3, js3, &v[0], &v[1], &v[2], wo, so, &v[3]) == DKG_E_ARG);
  CHECK(dkg_seat_pack(2, 3, js3, &v[0], &v[1], &v[2], wo, so, &v[3]) == DKG_E_ARG);
  CHECK(dkg_seat_pack(3, 3, nullptr, &v[0], &v[1], &v[2], wo, so, &v[3]) == DKG_E_ARG);
  CHECK(dkg_seat_pack(3, 3, js3, nullptr, &v[1], &v[2], wo, so, &v[3]) == DKG_E_ARG);
  CHECK(dkg_seat_pack(3, 3, js3, &v[0], &v[1], &v[2], nullptr, so, &v[3]) == DKG_E_ARG);
  CHECK(dkg_seat_pack(3, 3, js3, &v[0], &v[1], &v[2], wo, nullptr, &v[3]) == DKG_E_ARG);
  CHECK(dkg_seat_pack(3, 3, js3, &v[0], &v[1], &v[2], wo, so, nullptr) == DKG_E_ARG);
  v[3] = 9;
  CHECK(dkg_seat_pack(3, 0, nullptr, &v[0], &v[1], &v[2], nullptr, nullptr, &v[3]) == DKG_OK && v[3] == 0);
  CHECK(dkg_seat_pack(3, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == DKG_OK);
  dkgh::SeatPlan pl;
  CHECK(dkgh::seat_plan(5, 3, 3, cer3, js3, pl) == DKG_E_ARG);  // cer[2] >= B
  CHECK(dkgh::seat_plan(6, 3, 3, cer3, js3, pl) == DKG_OK && pl.cers.size() == 3);
  CHECK(dkgh::seat_plan(6, 3, 3, nullptr, js3, pl) == DKG_E_ARG);
  CHECK(dkgh::seat_plan(6, 3, 0, nullptr, nullptr, pl) == DKG_OK && pl.waves == 0 && pl.wave_seat.empty());
  puts("ok");
  return 0;
}
