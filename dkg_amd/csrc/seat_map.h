// Index arithmetic of the seats' evaluation (receivers.hip k_seat_horner, k_seat_chunks, k_seat_fold), read
// by the kernels, their launchers, the host packing (seat_pack.cpp) and the stand-alone checks
// (tools/seat_pack_check.cpp, tools/seat_chunks_check.cpp), so that the checks walk the code the GPU runs.
// dkg_seat_pack gives every wave one x (wdesc[2v]) and one tile of 64 dealers (wdesc[2v + 1]) and cuts its
// 64 lanes into 64 / W slots of W = 1 << wshift lanes (W = 64 for n >= 64, else the power of two that holds n):
//   wave v, lane l = slot W + i   ->   dealer d = tile 64 + i of seat wseat[v (64 / W) + slot]
// A lane is dead in an empty slot (SEAT_NONE) or with d >= n: it walks column 0 and stores no result.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DKG_SEAT_MAP_FN __host__ __device__ inline
#else
#define DKG_SEAT_MAP_FN inline
#endif

constexpr uint32_t SEAT_NONE = 0xffffffffu;  // wseat: no seat in this slot
constexpr size_t FOLD_DIG_WORDS = 17;        // a fold multiplier's NAF: +1 digits in words 0..7, -1 in 8..15, length

// log2 of a slot width the lane map takes (a power of two, at most 64), or -1
DKG_SEAT_MAP_FN int seat_wshift(uint32_t width) {
  int s = 0;
  while (s < 6 && (1u << s) < width) s++;
  return (1u << s) == width ? s : -1;
}

// the element of wseat that lane `lane` of wave v reads
DKG_SEAT_MAP_FN size_t seat_cell(uint32_t wshift, size_t v, uint32_t lane) {
  return (v << (6 - wshift)) + (lane >> wshift);
}

struct SeatLane {
  uint32_t slot, seat;  // slot of the wave; its seat, SEAT_NONE where empty
  size_t d;             // dealer
  bool live;            // a seat's dealer d < n
};
DKG_SEAT_MAP_FN SeatLane seat_lane(size_t n, uint32_t wshift, size_t v, uint32_t lane, const uint32_t* wdesc,
                                   const uint32_t* wseat) {
  SeatLane m;
  m.slot = lane >> wshift;
  m.seat = wseat[seat_cell(wshift, v, lane)];
  m.d = (size_t)wdesc[2 * v + 1] * 64 + (lane & ((1u << wshift) - 1u));
  m.live = m.seat != SEAT_NONE && m.d < n;
  return m;
}

// the lane's column of the position-major table over the decoded ceremonies (scol: seat -> ceremony slot)
DKG_SEAT_MAP_FN size_t seat_column(const SeatLane& m, size_t n, const uint32_t* scol) {
  return m.live ? (size_t)scol[m.seat] * n + m.d : 0;
}
// a live lane's element of the results R [seat n + d]
DKG_SEAT_MAP_FN size_t seat_result(const SeatLane& m, size_t n) { return (size_t)m.seat * n + m.d; }
// a lane's place wl among the 64 waves lanes of the launch, and element (chunk or fold value g, wl) of a
// partials buffer [G][lanes], lanes = 64 waves
DKG_SEAT_MAP_FN size_t seat_wave_lane(size_t v, uint32_t lane) { return v * 64 + lane; }
DKG_SEAT_MAP_FN size_t seat_partial(size_t lanes, size_t g, size_t wl) { return g * lanes + wl; }

// chunk u of N coefficients cut into chunks of L: [lo, hi), the last one may be short
struct ChunkSpan {
  size_t lo, hi;
};
DKG_SEAT_MAP_FN ChunkSpan chunk_span(size_t u, size_t L, size_t N) {
  const size_t lo = u * L;
  return {lo, lo + L < N ? lo + L : N};
}

// word offset of the record of (slot, stage s) in fold digit records [slots][stages][FOLD_DIG_WORDS]
DKG_SEAT_MAP_FN size_t fold_record(size_t slot, size_t stages, size_t s) {
  return (slot * stages + s) * FOLD_DIG_WORDS;
}
