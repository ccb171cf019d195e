// Banded lane map of k_stepping (kernels.hip): how a workgroup of S equal segments deals its lanes.
//
// Position p of a table is dead once p + j >= nrecv, and a wave stops issuing only when all of its
// 64 lanes are dead.  With 64 consecutive positions of ONE segment per wave, the waves that hold
// positions 0..63 of each segment issue for the whole launch.  Banded, wave w holds positions
// [wB, (w+1)B), B = 64 / S, of EVERY segment: it dies as a whole at step nrecv - wB, and a
// workgroup's waves die one after the other instead of in groups of S.
//
//   lane l = 64 w + s B + r   ->   segment s, position q = w B + r        (0 <= s < S, 0 <= r < B)
//
// A lane keeps its cached value in the LDS column of its lane index; the addend of position q is
// the column of the lane that holds q + 1 of the same segment: l + 1 inside a band, l + 65 - B at a
// band's end.  Within a group of 32 lanes the reads stay on distinct banks: the band ends read word
// 64 (w + 1) + s B, bank s B mod 32, which is the one bank the l + 1 reads of that band leave free.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DKG_STEP_MAP_FN __host__ __device__ inline
#else
#define DKG_STEP_MAP_FN inline
#endif

struct StepLane {
  int seg;   // segment of the workgroup (slot * nseg + piece-in-slot)
  int q;     // position within the segment
  int next;  // lane that holds position q + 1 of the segment (the segment's position 0 past the top)
};

// Band width B of a bs-lane workgroup whose slots of nseg segments (P lanes each, the last one Plast)
// fill it exactly, or 0 when the launch keeps the contiguous map: a lone segment, a ragged last
// piece (Plast != P: its bands would need padding lanes the slot does not have), slots that leave
// lanes over, or a segment count that does not divide a wave.
DKG_STEP_MAP_FN int step_band(int bs, int P, int nseg, int Plast) {
  if (P <= 0 || nseg <= 0 || Plast != P || bs % P) return 0;
  const int S = bs / P;
  if (S < 2 || S > 64 || 64 % S || S % nseg) return 0;
  return 64 / S;
}

DKG_STEP_MAP_FN StepLane step_band_lane(int l, int B, int bs) {
  const int w = l >> 6, s = (l & 63) / B, r = l % B;
  StepLane m;
  m.seg = s;
  m.q = w * B + r;
  m.next = r + 1 < B ? l + 1 : l + 65 - B;
  if (m.next >= bs) m.next = s * B;  // the top position adds nothing: any column of its own segment
  return m;
}
