// Stand-alone host check of the pair evaluation's plain C++: dkg_pair_eval_shape, the item-list builder
// (dkgh::distinct_places: distinct rows, distinct indices, slots) and the digit records of the fold's
// multipliers, meant to be built with -fsanitize=address,undefined and run on the CPU:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/pair_items_check.cpp dkg_amd/csrc/receiver_plan.cpp dkg_amd/csrc/host_crypto.cpp -o pair_items_check
// Exit status 0 and "ok" when every check holds.
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

int main() {
  // shapes: every N up to 5000 with the automatic chunk, every forced chunk up to 80 for N up to 300
  for (size_t N = 1; N <= 5000; N++) {
    uint32_t L, G, S;
    CHECK(dkg_pair_eval_shape(N - 1, 0, &L, &G, &S) == DKG_OK);
    CHECK(G >= 1 && G <= 64 && (size_t)L * G >= N && (size_t)(G - 1) * L < N && (1u << S) >= G && (S == 0 || (1u << (S - 1)) < G));
  }
  for (size_t N = 1; N <= 300; N++)
    for (int chunk = 1; chunk <= 80; chunk++) {
      uint32_t L = 0, G = 0, S = 0;
      const int rc = dkg_pair_eval_shape(N - 1, chunk, &L, &G, &S);
      const size_t l = (size_t)chunk < N ? (size_t)chunk : N, g = (N + l - 1) / l;
      CHECK((rc == DKG_OK) == (g <= 64));
      if (rc == DKG_OK) CHECK(L == l && G == g && (1u << S) >= G);
    }
  uint32_t v;
  CHECK(dkg_pair_eval_shape(7, 0, nullptr, &v, &v) == DKG_E_ARG);
  CHECK(dkg_pair_eval_shape(7, 0, &v, nullptr, &v) == DKG_E_ARG);
  CHECK(dkg_pair_eval_shape(7, 0, &v, &v, nullptr) == DKG_E_ARG);
  CHECK(dkg_pair_eval_shape(7, -1, &v, &v, &v) == DKG_E_ARG);
  CHECK(dkg_pair_eval_shape((size_t)-1, 0, &v, &v, &v) == DKG_E_ARG);

  // item lists: pseudo-random values with repeats; empty and one-element lists
  std::vector<uint32_t> distinct, place;
  dkgh::distinct_places(0, nullptr, distinct, place);
  CHECK(distinct.empty() && place.empty());
  uint32_t seed = 12345;
  for (size_t count : {(size_t)1, (size_t)2, (size_t)63, (size_t)1000, (size_t)20000}) {
    std::vector<uint32_t> in(count);
    for (auto& x : in) {
      seed = seed * 1664525u + 1013904223u;
      x = (seed >> 8) % (uint32_t)(count / 3 + 1) + ((seed >> 30) ? 0xfffff000u : 0u);
    }
    dkgh::distinct_places(count, in.data(), distinct, place);
    CHECK(place.size() == count && distinct.size() <= count);
    size_t next = 0;  // first appearances come in order
    for (size_t p = 0; p < count; p++) {
      CHECK(place[p] < distinct.size() && distinct[place[p]] == in[p]);
      if (place[p] == next) next++;
      CHECK(place[p] < next);
    }
    CHECK(next == distinct.size());
  }

  // digit records of the multipliers, as the runtime lays them out: [S][17] per distinct index
  for (size_t t : {(size_t)0, (size_t)7, (size_t)127, (size_t)511, (size_t)2047})
    for (uint32_t x : {1u, 2u, 683u, 1u << 24}) {
      uint32_t L, G, S;
      CHECK(dkg_pair_eval_shape(t, 0, &L, &G, &S) == DKG_OK);
      dkg_receiver_plan p;
      CHECK(dkg_receiver_plan_for(x, t, x, (int)L, &p) == DKG_OK);
      CHECK(p.stages == S);
      std::vector<uint32_t> rec(S * 17 + 1, 0);
      for (uint32_t k = 0; k < S; k++) {
        const int len = dkgh::naf256(p.mult[k], &rec[k * 17], &rec[k * 17 + 8], nullptr);
        rec[k * 17 + 16] = (uint32_t)len;
        CHECK(len >= 1 && len <= 256 && (x != 1 || len == 1));
      }
    }
  puts("ok");
  return 0;
}
