// Public shares of every party from the broadcast commitments on gfx950.  The verification key of party j
// is g s_j with s_j = sum_i s_ij over the dealers the ceremony ends with, and for a dealer whose round-3
// vector A_i is consistent, g s_ij = sum_k (j+1)^k A_i[k] (the round-4 equation, committee.rs:532-539).  So
//   public_share[j] = sum_k (j+1)^k S[k]  +  g sum_{i reconstructed} s_ij,   S[k] = sum_{i used} A_i[k]:
// ONE aggregated committed polynomial per ceremony, n (t + 1) additions, evaluated by the receivers'
// chunked evaluator (receivers.hip) with the ceremonies as its rows.  k_commit_colsum is that masked
// column sum; k_pubshare_out adds the disclosed term and encodes.
#include "kernels.h"
#include "points.h"

namespace dkgk {

namespace {

// the lane's value as a cached addend in its LDS column
DKG_DEV void colsum_publish(const ge_p3& p, uint32_t* q) {
  ge_cached c;
  ge_to_cached(c, p);
  lds_put_cached(q, c);
}

}  // namespace

// S[c][k] += sum of the slab's rows of ceremony c that are used, one 64-lane workgroup per column (c, k):
// block b is ceremony c = c0 + b / N, coefficient k = b % N.  The slab holds the global rows [r0, r0 + rows)
// (row c n + i = dealer i of ceremony c) decoded position-major, C [40][N][spad], so for a fixed k the
// dealers of a ceremony are contiguous and a wave's 40 loads are coalesced.  Lane l adds the rows lo + l,
// lo + l + 64, .. of [lo, hi) = the ceremony's rows inside the slab; the trip count is the wave's, and a
// position past hi rereads row lo and counts as the identity.  use[row] (null: all 1): 0 not used, 1 used,
// 2 used but absent; a row that is not used, absent or undecodable (rowok[col] == 0) contributes the
// identity, and a used row that is absent or undecodable clears ok[c] (every writer stores the same 0).
// The 64 partials then fold in six in-wave stages through the lanes' LDS columns -- lane u < w adds
// column u + w, the others their own, whose value is never read again -- and lane 0 adds the total into
// Sacc [40][N][bpad] (position-major over the ceremonies, the table k_recv_chunks reads as C).  One wave
// writes a given (c, k) per launch and the launches of a call are ordered on one stream: no atomics.
// Every addition is the complete formula.
__global__ __launch_bounds__(64, 3) void k_commit_colsum(size_t n, size_t N, size_t r0, size_t rows, size_t spad,
                                                         size_t c0, const uint32_t* __restrict__ C,
                                                         const uint8_t* __restrict__ rowok,
                                                         const uint8_t* __restrict__ use, size_t bpad,
                                                         uint32_t* Sacc, uint8_t* __restrict__ ok) {
  __shared__ uint32_t qs[PT_WORDS * 64];
  const uint32_t u = threadIdx.x;
  uint32_t* q = qs + u;
  const size_t c = c0 + blockIdx.x / N, k = blockIdx.x % N;
  const size_t lo = c * n > r0 ? c * n : r0;
  const size_t hi = (c + 1) * n < r0 + rows ? (c + 1) * n : r0 + rows;  // lo < hi: the ceremony meets the slab
  const size_t S = N * spad;
  ge_p3 acc, p;
  ge_identity(acc);
  bool bad = false;
#pragma unroll 1
  for (size_t base = lo; base < hi; base += 64) {
    const bool have = base + u < hi;
    const size_t row = have ? base + u : lo, col = row - r0;
    const uint8_t m = use ? use[row] : (uint8_t)1, dec = rowok[col];
    bad |= have && (m == 2 || (m == 1 && !dec));
    pt_load(p, C, S, k * spad + col);
    pt_or_identity(p, have && m == 1 && dec);
    colsum_publish(p, q);
    ge_add_lds(acc, acc, q, false);
  }
#pragma unroll 1
  for (uint32_t w = 32; w; w >>= 1) {
    colsum_publish(acc, q);
    __syncthreads();  // every column holds its lane's partial
    ge_add_lds(acc, acc, u < w ? q + w : q, false);
    __syncthreads();  // the partners are read before the next stage overwrites the columns
  }
  if (bad && k == 0) ok[c] = 0;
  if (u != 0) return;
  // the running sum: read and written through the same pointer
  const size_t Sb = N * bpad, e = k * bpad + c;
#pragma unroll
  for (int w = 0; w < PT_WORDS; w++) pt_word(p, w) = Sacc[(size_t)w * Sb + e];
  colsum_publish(acc, q);
  ge_add_lds(p, p, q, false);
#pragma unroll
  for (int w = 0; w < PT_WORDS; w++) Sacc[(size_t)w * Sb + e] = pt_word(p, w);
}

// V[c][m] = the encoding of R[m B + c] (point-major, the evaluator's results with the ceremonies as rows)
// + G[c M + m] (SoA at stride B M: g times the disclosed shares; null: none)
__global__ __launch_bounds__(256) void k_pubshare_out(size_t B, size_t M, const uint32_t* __restrict__ R,
                                                      const uint32_t* __restrict__ G, uint32_t* __restrict__ V) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B * M) return;
  const size_t c = e / M, m = e % M;
  ge_p3 pt;
  pt_load_aos(pt, R, m * B + c);
  if (G) {
    ge_p3 g;
    pt_load(g, G, B * M, e);
    ge_cached gc;
    ge_to_cached(gc, g);
    ge_add(pt, pt, gc);
  }
  uint32_t w[8];
  ristretto_encode(w, pt);
  st_words8(V + 8 * e, w);
}

void commit_colsum(size_t n, size_t N, size_t r0, size_t rows, size_t spad, const uint32_t* C, const uint8_t* rowok,
                   const uint8_t* use, size_t bpad, uint32_t* Sacc, uint8_t* ok, hipStream_t stream) {
  if (!n || !N || !rows || spad < rows) return;
  const size_t c0 = r0 / n, c1 = (r0 + rows - 1) / n;
  if (c1 >= bpad || (c1 - c0 + 1) > 0x7fffffffu / N) return;  // grid.x
  hipLaunchKernelGGL(k_commit_colsum, dim3((unsigned)((c1 - c0 + 1) * N)), dim3(64), 0, stream, n, N, r0, rows, spad,
                     c0, C, rowok, use, bpad, Sacc, ok);
}

void pubshare_out(size_t B, size_t M, const uint32_t* R, const uint32_t* G, uint32_t* V, hipStream_t stream) {
  if (!B || !M) return;
  hipLaunchKernelGGL(k_pubshare_out, dim3((unsigned)((B * M + 255) / 256)), dim3(256), 0, stream, B, M, R, G, V);
}

}  // namespace dkgk
