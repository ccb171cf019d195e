// Stand-alone host check of the seats' chunked evaluation (receivers.hip k_seat_chunks / k_seat_fold):
// the chunk and fold index arithmetic of seat_map.h -- the functions the kernels themselves run -- walked lane
// by lane, from dkgh::seat_plan's descriptors and dkg_seat_eval_shape, as the runtime (seats_eval) launches
// it.  Every Q read must be in bounds and written earlier in the same call, every xslot in range, and every
// live (seat, dealer) must get exactly one R store, dead lanes none.  Meant to be built with
// -fsanitize=address,undefined and run on the CPU:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/seat_chunks_check.cpp dkg_amd/csrc/seat_pack.cpp dkg_amd/csrc/receiver_plan.cpp \
//       dkg_amd/csrc/host_crypto.cpp -o seat_chunks_check
// Exit status 0 and "ok" when every check holds.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
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

static uint32_t seed = 88172645u;
static uint32_t rnd() {
  seed = seed * 1664525u + 1013904223u;
  return seed >> 8;
}

// one seat list at one chunk (0: the rule's): the launches of seats_eval replayed on an epoch table --
// stamp[b][e] = the launch that last wrote element e of buffer b in this call, 0 for never
static int run(size_t B, size_t n, size_t t, const std::vector<uint32_t>& cer, const std::vector<uint32_t>& js,
               int chunk) {
  const size_t S = js.size(), N = t + 1;
  dkgh::SeatPlan pl;
  CHECK(dkgh::seat_plan(B, n, S, cer.data(), js.data(), pl) == DKG_OK);
  const size_t waves = pl.waves, lanes = 64 * waves, W = pl.width;
  CHECK(seat_wshift((uint32_t)W) >= 0);  // the launchers' validity test
  const uint32_t wshift = (uint32_t)seat_wshift((uint32_t)W);
  const uint32_t x_max = *std::max_element(pl.seat_x.begin(), pl.seat_x.end());
  uint32_t L = 0, G = 0, stages = 0;
  uint64_t scratch = 0;
  CHECK(dkg_seat_eval_shape(n, t, waves, x_max, chunk, &L, &G, &stages, &scratch) == DKG_OK);
  CHECK(L >= 1 && L <= N && G == (N + L - 1) / L && ((size_t)1 << stages) >= G && (stages == 0 || (1u << (stages - 1)) < G));
  CHECK(scratch == (G > 1 ? (uint64_t)2 * 160 * G * 64 * waves : 0));
  if (chunk == 0) CHECK(scratch <= ((uint64_t)1 << 30));
  if (G == 1) return 0;  // the serial kernel: tools/seat_pack_check.cpp
  // the host's records: one per (distinct x, stage), the waves name their x's
  std::vector<uint32_t> wx(waves), xs, xslot;
  for (size_t v = 0; v < waves; v++) wx[v] = pl.wave_desc[2 * v];
  dkgh::distinct_places(waves, wx.data(), xs, xslot);
  const size_t dig_words = fold_record(xs.size(), stages, 0);
  for (size_t k = 0; k < xs.size(); k++) {
    dkg_receiver_plan p;
    CHECK(dkg_receiver_plan_for(n, t, xs[k], (int)L, &p) == DKG_OK && p.stages == stages);
    for (uint32_t s = 0; s < stages; s++) CHECK(p.arity[s] == 2);
  }
  for (size_t v = 0; v < waves; v++) CHECK(xslot[v] < xs.size() && xs[xslot[v]] == wx[v]);
  // Q[0], Q[1]: words [40][G][lanes] each, carved from one allocation of `scratch` bytes
  const size_t half_words = (size_t)(scratch / 8);
  CHECK(2 * half_words * 4 == scratch);
  std::vector<uint32_t> stamp[2];
  stamp[0].assign((size_t)G * lanes, 0);  // one entry per point: the 40 words share index arithmetic (word w at
  stamp[1].assign((size_t)G * lanes, 0);  // w * stride + e, e < stride, checked below)
  auto in_bounds = [&](size_t stride, size_t e) { return e < stride && 39 * stride + e < half_words; };
  const size_t cols = (pl.cers.size() * n + 63) / 64 * 64;
  uint32_t launch = 1;
  // k_seat_chunks, grid (waves, G)
  for (size_t v = 0; v < waves; v++)
    for (size_t u = 0; u < G; u++)
      for (uint32_t l = 0; l < 64; l++) {
        CHECK(seat_cell(wshift, v, l) < pl.wave_seat.size());
        const SeatLane m = seat_lane(n, wshift, v, l, pl.wave_desc.data(), pl.wave_seat.data());
        if (m.live) CHECK(m.seat < S);
        CHECK(seat_column(m, n, pl.seat_col.data()) < cols);
        const ChunkSpan ch = chunk_span(u, L, N);
        CHECK(ch.lo < ch.hi && ch.hi <= N);  // C reads (hi - 1) * cols + col .. lo * cols + col of N * cols
        const size_t e = seat_partial(lanes, u, seat_wave_lane(v, l));
        CHECK(in_bounds((size_t)G * lanes, e));
        CHECK(stamp[0][e] == 0);  // written once
        stamp[0][e] = launch;
      }
  // k_seat_fold, one launch per stage, grid (waves, Gout)
  std::vector<uint8_t> stored(S * n, 0);
  size_t Gin = G;
  for (uint32_t s = 0; s < stages; s++) {
    launch++;
    const size_t Gout = (Gin + 1) / 2;
    CHECK(Gin >= 2);
    std::vector<uint32_t>& in = stamp[s & 1];
    std::vector<uint32_t>& out = stamp[(s + 1) & 1];
    for (size_t v = 0; v < waves; v++) {
      // seats_eval passes ddig + fold_record(0, stages, s) and the stride fold_record(1, stages, 0)
      const size_t rec = fold_record(0, stages, s) + (size_t)xslot[v] * fold_record(1, stages, 0);
      CHECK(rec + FOLD_DIG_WORDS <= dig_words);
      for (size_t w = 0; w < Gout; w++)
        for (uint32_t l = 0; l < 64; l++) {
          const size_t lane = seat_wave_lane(v, l);
          const size_t e0 = seat_partial(lanes, 2 * w, lane), e1 = seat_partial(lanes, 2 * w + 1, lane);
          CHECK(in_bounds(Gin * lanes, e0) && in[e0] == launch - 1);  // what the launch before wrote
          if (2 * w + 1 < Gin) CHECK(in_bounds(Gin * lanes, e1) && in[e1] == launch - 1);
          if (Gout != 1) {
            const size_t e = seat_partial(lanes, w, lane);
            CHECK(in_bounds(Gout * lanes, e));
            CHECK(out[e] != launch);  // once per launch
            out[e] = launch;
            continue;
          }
          const SeatLane m = seat_lane(n, wshift, v, l, pl.wave_desc.data(), pl.wave_seat.data());
          if (!m.live) continue;  // dead: nothing stored
          CHECK(m.seat < S && m.d < n && !stored[seat_result(m, n)]);
          stored[seat_result(m, n)] = 1;
        }
    }
    Gin = Gout;
  }
  CHECK(Gin == 1);
  for (uint8_t v : stored) CHECK(v);
  return 0;
}

int main() {
  struct Shape {
    size_t n, t;
  };
  const Shape shapes[] = {{10, 4}, {3, 1}, {2, 0}, {16, 7}, {64, 31}, {70, 34}, {130, 64}, {256, 127}, {1024, 511}};
  for (const Shape& sh : shapes) {
    const size_t n = sh.n, N = sh.t + 1;
    for (size_t S : {(size_t)1, (size_t)2, (size_t)9, (size_t)65}) {
      if (n >= 256 && S > 9) continue;
      const size_t B = S / 2 + 1;
      std::vector<uint32_t> cer(S), js(S);
      for (int kind = 0; kind < 3; kind++) {
        for (size_t p = 0; p < S; p++) {
          cer[p] = rnd() % (uint32_t)B;
          js[p] = kind == 0 ? rnd() % (uint32_t)n : kind == 1 ? (uint32_t)(n - 1) : rnd() % (uint32_t)(n < 3 ? n : 3);
        }
        for (int chunk : {0, 1, 2, 3, 4, 5, 8, 9, 16, 33, 64, (int)N - 1, (int)N, (int)N + 5})
          if (chunk >= 0 && run(B, n, sh.t, cer, js, chunk)) return 1;
      }
    }
  }
  // arguments
  uint32_t L, G, st;
  uint64_t sb;
  CHECK(dkg_seat_eval_shape(0, 4, 1, 1, 0, &L, &G, &st, &sb) == DKG_E_ARG);
  CHECK(dkg_seat_eval_shape(10, 4, 0, 1, 0, &L, &G, &st, &sb) == DKG_E_ARG);
  CHECK(dkg_seat_eval_shape(10, 4, 1, 0, 0, &L, &G, &st, &sb) == DKG_E_ARG);
  CHECK(dkg_seat_eval_shape(10, 4, 1, 11, 0, &L, &G, &st, &sb) == DKG_E_ARG);
  CHECK(dkg_seat_eval_shape(10, 4, 1, 10, -1, &L, &G, &st, &sb) == DKG_E_ARG);
  CHECK(dkg_seat_eval_shape(10, 4, 1, 10, 0, nullptr, &G, &st, &sb) == DKG_E_ARG);
  CHECK(dkg_seat_eval_shape(10, 4, 1, 10, 0, &L, &G, &st, nullptr) == DKG_E_ARG);
  CHECK(dkg_seat_eval_shape(100000, 70000, 1, 3, 1, &L, &G, &st, &sb) == DKG_E_ARG);  // G > 65535
  puts("ok");
  return 0;
}
