// Device helpers and build knobs shared by the width-4 decryption chains of hybrid.hip (one ceremony)
// and hybrid_batch.hip (batches): moved here unchanged from hybrid.hip.
#pragma once
#include "points.h"

// DKG_DEC_W4_WAVES: the launch bound's waves per SIMD; DKG_DEC_IL: paired products in the chain's
// doublings and additions (ge25519.h IL).  3 waves at <= 168 VGPRs with pairs (no scratch in the
// chain) against 4 at 128 without (24 VGPRs spilled in the table setup): full mode 111.6-111.7 against
// 112.8-113.0 ms per ceremony, k_dec_mul_w4 18.7-19.1 against 19.5-19.9 ms (profiles/r06_pair_ab.txt).
#ifndef DKG_DEC_W4_WAVES
#define DKG_DEC_W4_WAVES 3
#endif
#ifndef DKG_DEC_IL
#define DKG_DEC_IL 1
#endif
typedef __attribute__((address_space(3))) uint32_t dec_lds_u32;
typedef __attribute__((address_space(1))) uint32_t dec_g_u32;

// words 0..N-1 (64 lanes each) from sg into the LDS rows at q.  The instruction's immediate offset
// (K * 256 B) moves BOTH addresses -- the global one and the LDS one (M0 + offset + lane * 4) -- so
// the LDS base stays q for every word of the group.
template <int N, int K = 0>
DKG_DEV void glds_words(const dec_g_u32* sg, uint32_t* q) {
  if constexpr (K < N) {
    __builtin_amdgcn_global_load_lds(sg, (dec_lds_u32*)q, 4, K * 256, 0);
    glds_words<N, K + 1>(sg, q);
  }
}

// The width-4 window's odd multiples live in a global table of one 40-KB slot per wave of a launch
// (T, indexed by the wave's place in its grid).  Launches are capped at DEC_TAB_WAVES waves -- eight
// rounds of a full chip's resident waves -- and cover the recipients in slices, back to back on the
// stream, so the table never exceeds DEC_TAB_WAVES slots (1.3 GB) whatever n is (n = 1024: one
// launch; n = 4096: 16 launches instead of one grid of 524,288 waves and a 21-GB table).  A cap of
// 16,384 (two launches at n = 1024) cost 0.8-1.0 ms there (profiles/r04_dec_slices_ab.txt).
#ifndef DKG_DEC_TAB_WAVES
#define DKG_DEC_TAB_WAVES 32768
#endif
constexpr size_t DEC_TAB_WAVES = DKG_DEC_TAB_WAVES;
