// One party's share checks on gfx950: P_i(x) = sum_k x^k C_i[k] for a FEW receiver indices x and
// all dealers i (the shared-scalar case of vartime_multiscalar_multiplication, committee.rs:287-296
// and :532-539, as Phases<Phase1>::proceed / Phases<Phase3>::proceed run it for one party).
// k_horner (kernels.hip) walks the t + 1 coefficients as ONE dependent chain per dealer; here the
// polynomial is cut into G chunks of L coefficients that are walked side by side,
//   stage 1  Q_u = sum_{k < L} x^k C[uL + k]            lane = (dealer, chunk u, receiver)
//   stage 2  groups of r consecutive partials folded by Horner in y_s (y_0 = x^L, y_{s+1} = y_s^r),
// so the chain is L - 1 small multiplications and one long one per fold stage.  Every multiplier is
// the same for all dealers, hence uniform over the wave (dealers run along the wave); the long ones
// come from the host as signed digits (dkg_receiver_plan_for).  Every addition is the complete
// formula, so identity rows, equal operands and torsion representatives need no redo.
// k_pair_eval gives one wave to one (row, index) pair; k_seat_horner walks the seats (ceremony, party) of
// one operator serially, seats of equal x side by side in a wave (dkg_seat_pack); k_seat_chunks and
// k_seat_fold are stages 1 and 2 on that placement, for the seats of large committees.
// Built twice like kernels.hip (dkg_amd/Makefile): namespace dkgk, and dkgk_ilp with DKG_FE_ILP.
#ifdef DKG_FE_ILP
#define dkgk dkgk_ilp
#endif
#include "kernels.h"
#include "points.h"
#include "seat_map.h"

namespace dkgk {

namespace {

// lane's cached addend in the wave's LDS slot, then y += it
DKG_DEV void add_point_lds(ge_p3& y, const ge_p3& c, uint32_t* q) {
  ge_cached cc;
  ge_to_cached(cc, c);
  lds_put_cached(q, cc);
  ge_add_lds(y, y, q, false);
}

// y = m y for a wave-uniform small m (small_recode's chain; m = 1 is the empty chain); q clobbered
DKG_DEV void recv_mul_small(ge_p3& y, uint32_t pos, uint32_t neg, int len, uint32_t* q) {
  if (len <= 1) return;
  {
    ge_cached xc;
    ge_to_cached(xc, y);
    lds_put_cached(q, xc);
  }
#pragma unroll 1
  for (int i = len - 2; i >= 0; i--) {
    const uint32_t bit = 1u << i;
    const bool nz = ((pos | neg) & bit) != 0;
    ge_dbl_lean(y, y, nz || i == 0);
    if (nz) ge_add_lds(y, y, q, (neg & bit) != 0, 64, i == 0);  // T only for the result
  }
}

// the chain of recv_mul_long after its first step: q holds cached(y) of before the chain, len >= 2
DKG_DEV void recv_chain_long(ge_p3& y, const uint32_t* __restrict__ dg, int len, const uint32_t* q) {
#pragma unroll 1
  for (int i = len - 2; i >= 0; i--) {
    const uint32_t bit = 1u << (i & 31);
    const uint32_t p = dg[i >> 5] & bit, n = dg[8 + (i >> 5)] & bit;
    const bool nz = (p | n) != 0;
    ge_dbl_lean(y, y, nz || i == 0);
    if (nz) ge_add_lds(y, y, q, n != 0, 64, i == 0);
  }
}

// y = m y for a wave-uniform multiplier of up to 255 bits: dg = NAF digits, +1 in words 0..7, -1 in
// words 8..15, length in word 16 (top digit +1 at length - 1)
DKG_DEV void recv_mul_long(ge_p3& y, const uint32_t* __restrict__ dg, uint32_t* q) {
  const int len = (int)dg[16];
  if (len <= 1) return;
  {
    ge_cached xc;
    ge_to_cached(xc, y);
    lds_put_cached(q, xc);
  }
  recv_chain_long(y, dg, len, q);
}

// final values: point-major R[m * ndealers + d] (what check and k_recv_encode read)
DKG_DEV void recv_store(bool last, uint32_t* __restrict__ out, size_t ostride, size_t oidx, uint32_t* __restrict__ R,
                        size_t ridx, bool live, const ge_p3& acc) {
  if (!last) pt_store(out, ostride, oidx, acc);
  else if (live) pt_store_aos(R, ridx, acc);
}

// acc = sum over k in [lo, hi) of x^(k - lo) C[k] for one column of a position-major table, from the top
// down: coefficient k of the column is element k * kstride + col at word stride S; (pos, neg, len) is
// small_recode(x), q the lane's LDS slot.  hi - lo - 1 steps; a chunk of one coefficient has none.
DKG_DEV void chunk_walk(ge_p3& acc, const uint32_t* __restrict__ C, size_t S, size_t kstride, size_t col, size_t lo,
                        size_t hi, uint32_t pos, uint32_t neg, int len, uint32_t* q) {
  ge_p3 c;
  pt_load(acc, C, S, (hi - 1) * kstride + col);
#pragma unroll 1
  for (size_t k = hi - 1; k-- > lo;) {
    recv_mul_small(acc, pos, neg, len, q);
    pt_load(c, C, S, k * kstride + col);
    add_point_lds(acc, c, q);
  }
}

}  // namespace

// Stage 1.  C position-major [40][N][npad]; xs[m] = receiver index (1-based) of slot m0 + blockIdx.z.
// Q [40][Ms][G][npad] (dealers minor), or R when G == 1.
__global__ __launch_bounds__(64, 3) void k_recv_chunks(size_t ndealers, size_t npad, size_t N, size_t L, size_t G,
                                                       const uint32_t* __restrict__ C,
                                                       const uint32_t* __restrict__ xs, size_t m0,
                                                       uint32_t* __restrict__ Q, uint32_t* __restrict__ R) {
  __shared__ uint32_t qs[PT_WORDS * 64];
  uint32_t* q = qs + threadIdx.x;
  const size_t d = (size_t)blockIdx.x * 64 + threadIdx.x;  // < npad: the grid is npad / 64 wide
  const size_t u = blockIdx.y, m = blockIdx.z;
  const uint32_t x = xs[m0 + m];
  uint32_t pos, neg;
  const int len = small_recode(x, pos, neg);
  const ChunkSpan ch = chunk_span(u, L, N);
  ge_p3 acc;
  chunk_walk(acc, C, N * npad, npad, d, ch.lo, ch.hi, pos, neg, len, q);
  recv_store(G == 1, Q, (size_t)gridDim.z * G * npad, (m * G + u) * npad + d, R, (m0 + m) * ndealers + d,
             d < ndealers, acc);
}

// Stage 2, one fold stage: out[v] = sum_{i < r} y^i in[v r + i] over the partials that exist
// (Gin need not be a multiple of r).  dg: the stage's digits of slot m0 + blockIdx.z (FOLD_DIG_WORDS words,
// stride dstride).
__global__ __launch_bounds__(64, 3) void k_recv_fold(size_t ndealers, size_t npad, size_t Gin, size_t r,
                                                     const uint32_t* __restrict__ in,
                                                     const uint32_t* __restrict__ digits, size_t dstride, size_t m0,
                                                     uint32_t* __restrict__ out, uint32_t* __restrict__ R) {
  __shared__ uint32_t qs[PT_WORDS * 64];
  uint32_t* q = qs + threadIdx.x;
  const size_t d = (size_t)blockIdx.x * 64 + threadIdx.x;
  const size_t v = blockIdx.y, m = blockIdx.z, Gout = gridDim.y;
  const uint32_t* dg = digits + (m0 + m) * dstride;
  const size_t first = v * r, cnt = first + r <= Gin ? r : Gin - first;
  const size_t S = (size_t)gridDim.z * Gin * npad, base = (m * Gin + first) * npad + d;
  ge_p3 acc, c;
  pt_load(acc, in, S, base + (cnt - 1) * npad);
#pragma unroll 1
  for (size_t i = cnt - 1; i-- > 0;) {
    recv_mul_long(acc, dg, q);
    pt_load(c, in, S, base + i * npad);
    add_point_lds(acc, c, q);
  }
  recv_store(Gout == 1, out, (size_t)gridDim.z * Gout * npad, (m * Gout + v) * npad + d, R, (m0 + m) * ndealers + d,
             d < ndealers, acc);
}

// P_row(x) for a LIST of (row, index) items, one 64-lane workgroup per item: the index is uniform over
// the wave, and the lanes hold G <= 64 chunks of L coefficients of that one polynomial (G = ceil(N / L),
// S = ceil(log2 G): dkg_pair_eval_shape).  Item b: c = list[b] (b itself with a null list), row
// crow[c] - 1 of the decoded commitments Eext (element row * N + k, as k_cmp_horner reads them), index
// x = xs[c], digit records digits[slot[b]][S][FOLD_DIG_WORDS] of the multipliers y_s = x^(L 2^s).
//   stage 1  lane u walks coefficients [uL, min(uL + L, N)) by Horner in x: L - 1 steps in every lane; a
//            position past the row's end, and every position of a lane >= G, is the identity
//   fold s   V_u = y_s V_u + V_(u - 2^s) in the lanes whose bit s is set: recv_mul_long leaves cached(V_u)
//            of BEFORE the multiplication in the lane's LDS column, which is what lane u + 2^s adds.  The
//            other lanes add their own column; their value is never read again.  The result migrates
//            upward and ends in lane 2^S - 1, which alone stores it.
// R point-major [c][40], the format of k_cmp_horner's results.
__global__ __launch_bounds__(64, 3) void k_pair_eval(const uint32_t* __restrict__ list,
                                                     const uint32_t* __restrict__ xs,
                                                     const uint32_t* __restrict__ crow,
                                                     const uint32_t* __restrict__ slot,
                                                     const uint32_t* __restrict__ Eext, size_t stride, size_t N,
                                                     uint32_t L, uint32_t G, uint32_t S,
                                                     const uint32_t* __restrict__ digits, uint32_t* __restrict__ R) {
  __shared__ uint32_t qs[PT_WORDS * 64];
  const uint32_t u = threadIdx.x;
  uint32_t* q = qs + u;
  const size_t b = blockIdx.x;
  const size_t c = list ? list[b] : b;
  const uint32_t x = xs[c];
  const size_t row = (size_t)(crow[c] - 1) * N;
  uint32_t pos, neg;
  const int len = small_recode(x, pos, neg);
  const size_t lo = (size_t)u * L;
  ge_p3 acc, e;
  {
    const size_t k = lo + L - 1;
    const bool have = u < G && k < N;
    pt_load(acc, Eext, stride, row + (have ? k : 0));  // no lane reads past its row
    pt_or_identity(acc, have);
  }
#pragma unroll 1
  for (uint32_t i = L - 1; i-- > 0;) {
    recv_mul_small(acc, pos, neg, len, q);
    const size_t k = lo + i;
    const bool have = u < G && k < N;
    pt_load(e, Eext, stride, row + (have ? k : 0));
    pt_or_identity(e, have);
    add_point_lds(acc, e, q);
  }
#pragma unroll 1
  for (uint32_t s = 0; s < S; s++) {
    const uint32_t* dg = digits + fold_record(slot[b], S, s);
    {  // recv_mul_long, whose first step is skipped by the empty chain (y_s = 1 at x = 1): the column
       // is written either way, since the partner reads it
      ge_cached cc;
      ge_to_cached(cc, acc);
      lds_put_cached(q, cc);
    }
    recv_chain_long(acc, dg, (int)dg[16], q);
    __syncthreads();  // every column holds its lane's unmultiplied value
    const uint32_t w = 1u << s;
    ge_add_lds(acc, acc, (u & w) ? qs + (u - w) : q, false);
    __syncthreads();  // the partners are read before the next stage overwrites the columns
  }
  if (u == (1u << S) - 1) pt_store_aos(R, c, acc);
}

// P_i(x) for the SEATS (ceremony, party) of one operator, one 64-lane workgroup per wave of dkg_seat_pack's
// placement.  Every polynomial of a seat is evaluated at the seat's x = j + 1, and the host packs only
// seats of equal x into one wave, so the multiplier is wave-uniform as in k_recv_chunks: the serial walk
// acc = x acc + C[k] over the N coefficients, no fold.  Wave v evaluates at x = wdesc[2v]; seat_map.h has
// the lane map (seat_lane) and the lane's column of the position-major table C [40][N][cols] over the
// decoded ceremonies (seat_column).  A dead lane walks column 0 and stores nothing.
// R point-major [seat n + d][40].
__global__ __launch_bounds__(64, 3) void k_seat_horner(size_t n, size_t N, size_t cols, uint32_t wshift,
                                                       const uint32_t* __restrict__ wdesc,
                                                       const uint32_t* __restrict__ wseat,
                                                       const uint32_t* __restrict__ scol,
                                                       const uint32_t* __restrict__ C, uint32_t* __restrict__ R) {
  __shared__ uint32_t qs[PT_WORDS * 64];
  uint32_t* q = qs + threadIdx.x;
  const size_t v = blockIdx.x;
  const SeatLane m = seat_lane(n, wshift, v, threadIdx.x, wdesc, wseat);
  const size_t col = seat_column(m, n, scol);
  uint32_t pos, neg;
  const int len = small_recode(wdesc[2 * v], pos, neg);
  ge_p3 acc;
  chunk_walk(acc, C, N * cols, cols, col, 0, N, pos, neg, len, q);
  if (m.live) pt_store_aos(R, seat_result(m, n), acc);
}

// k_seat_horner cut into G = ceil(N / L) chunks that are walked side by side, for the seats of large
// committees whose serial walk leaves the device empty: grid (waves, G), block (v, u) has k_seat_horner's
// lane map and walks coefficients [uL, min(uL + L, N)) of its column from the top down (the last chunk
// may be short; L = 1 has no step).  The partial goes to Q [40][G][64 waves], lanes minor: lane
// v 64 + threadIdx.x of chunk u, dead lanes (which walk column 0) included, so that k_seat_fold reads
// only what was written.  The exactness note of k_recv_chunks holds unchanged: every addition is
// complete, and a multiplier may be any representative mod l since the operands lie in 2E.
__global__ __launch_bounds__(64, 3) void k_seat_chunks(size_t n, size_t N, size_t cols, uint32_t wshift, size_t L,
                                                       const uint32_t* __restrict__ wdesc,
                                                       const uint32_t* __restrict__ wseat,
                                                       const uint32_t* __restrict__ scol,
                                                       const uint32_t* __restrict__ C, uint32_t* __restrict__ Q) {
  __shared__ uint32_t qs[PT_WORDS * 64];
  uint32_t* q = qs + threadIdx.x;
  const size_t v = blockIdx.x, u = blockIdx.y, G = gridDim.y, lanes = (size_t)gridDim.x * 64;
  const SeatLane m = seat_lane(n, wshift, v, threadIdx.x, wdesc, wseat);
  const size_t col = seat_column(m, n, scol);
  uint32_t pos, neg;
  const int len = small_recode(wdesc[2 * v], pos, neg);
  const ChunkSpan ch = chunk_span(u, L, N);
  ge_p3 acc;
  chunk_walk(acc, C, N * cols, cols, col, ch.lo, ch.hi, pos, neg, len, q);
  pt_store(Q, G * lanes, seat_partial(lanes, u, seat_wave_lane(v, threadIdx.x)), acc);
}

// One fold stage of the seats' partials, arity 2: grid (waves, Gout = ceil(Gin / 2)),
// out[v'] = y in[2 v' + 1] + in[2 v'], or in[2 v'] alone where the upper partial does not exist (odd
// Gin).  y = x^(L 2^stage) mod l is uniform over the wave but differs from wave to wave: wave v reads
// the record (recv_mul_long's format, FOLD_DIG_WORDS words) digits[xslot[v] * dstride ..] of its x at this
// stage; at x = 1 the chain is empty.  in [40][Gin][64 waves], out [40][Gout][64 waves]; the last stage (Gout == 1)
// stores the live lanes to R [seat n + d][40] point-major instead, dead lanes nothing.
__global__ __launch_bounds__(64, 3) void k_seat_fold(size_t n, uint32_t wshift, size_t Gin,
                                                     const uint32_t* __restrict__ wdesc,
                                                     const uint32_t* __restrict__ wseat,
                                                     const uint32_t* __restrict__ xslot,
                                                     const uint32_t* __restrict__ digits, size_t dstride,
                                                     const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                     uint32_t* __restrict__ R) {
  __shared__ uint32_t qs[PT_WORDS * 64];
  uint32_t* q = qs + threadIdx.x;
  const size_t v = blockIdx.x, w = blockIdx.y, Gout = gridDim.y, lanes = (size_t)gridDim.x * 64;
  const size_t lane = seat_wave_lane(v, threadIdx.x), S = Gin * lanes;
  ge_p3 acc, c;
  if (2 * w + 1 < Gin) {
    pt_load(acc, in, S, seat_partial(lanes, 2 * w + 1, lane));
    recv_mul_long(acc, digits + (size_t)xslot[v] * dstride, q);
    pt_load(c, in, S, seat_partial(lanes, 2 * w, lane));
    add_point_lds(acc, c, q);
  } else {
    pt_load(acc, in, S, seat_partial(lanes, 2 * w, lane));
  }
  if (Gout != 1) {
    pt_store(out, Gout * lanes, seat_partial(lanes, w, lane), acc);
    return;
  }
  const SeatLane m = seat_lane(n, wshift, v, threadIdx.x, wdesc, wseat);
  if (m.live) pt_store_aos(R, seat_result(m, n), acc);
}

// sok[p n + i] = dok[scol[p] n + i] (and extra[p n + i], may be null): dealer i's data decodes for seat p
__global__ __launch_bounds__(256) void k_seat_ok(size_t S, size_t n, const uint32_t* __restrict__ scol,
                                                 const uint8_t* __restrict__ dok, const uint8_t* __restrict__ extra,
                                                 uint8_t* __restrict__ sok) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= S * n) return;
  const size_t p = e / n, i = e % n;
  sok[e] = dok[(size_t)scol[p] * n + i] && (!extra || extra[e]);
}

// k_recv_decide for seats: dec [S][n] holds the group equation's outcome; seat p = party sx[p] - 1 of
// ceremony scer[p], whose qualified set is qualified[scer[p] n ..] (may be null).  The same order:
// undecodable data (sok), then SKIPPED, then SELF.
__global__ __launch_bounds__(256) void k_seat_decide(size_t S, size_t n, int round, const uint32_t* __restrict__ sx,
                                                     const uint32_t* __restrict__ scer,
                                                     const uint8_t* __restrict__ sok,
                                                     const uint8_t* __restrict__ qualified,
                                                     uint8_t* __restrict__ dec) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= S * n) return;
  const size_t p = e / n, i = e % n;
  uint8_t v = sok[e] ? dec[e] : (round == 2 ? 4 : 0);
  if (qualified && !qualified[(size_t)scer[p] * n + i]) v = 3;
  if ((uint32_t)(i + 1) == sx[p]) v = 2;
  dec[e] = v;
}

// ok[p] = rowok[crow[p] - 1]: the items of k_pair_eval whose row decodes
__global__ __launch_bounds__(256) void k_pair_ok(size_t cnt, const uint32_t* __restrict__ crow,
                                                 const uint8_t* __restrict__ rowok, uint8_t* __restrict__ ok) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < cnt) ok[p] = rowok[crow[p] - 1];
}

// Decisions [M][n] from the group equation's outcome eq[m * n + i] (check with an all-ones mask and no
// self index): undecodable rows (MISSING in round 2, REJECT in round 4), SELF where i == js[m], and
// SKIPPED for a dealer outside the qualified set (round 4, committee.rs:522), in check's order.
__global__ __launch_bounds__(256) void k_recv_decide(size_t M, size_t n, int round, const uint32_t* __restrict__ xs,
                                                     const uint8_t* __restrict__ dok,
                                                     const uint8_t* __restrict__ qualified,
                                                     uint8_t* __restrict__ dec) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= M * n) return;
  const size_t m = p / n, i = p % n;
  uint8_t v = dok[i] ? dec[p] : (round == 2 ? 4 : 0);
  if (qualified && !qualified[i]) v = 3;
  if ((uint32_t)(i + 1) == xs[m]) v = 2;
  dec[p] = v;
}

// P [M][D][8 words] = the encodings of R [M * D][40] (point-major), zero where row i did not decode
__global__ __launch_bounds__(256) void k_recv_encode(size_t M, size_t D, const uint32_t* __restrict__ R,
                                                     const uint8_t* __restrict__ dok, uint32_t* __restrict__ P) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= M * D) return;
  ge_p3 pt;
  pt_load_aos(pt, R, p);
  uint32_t w[8];
  ristretto_encode(w, pt);
  if (!dok[p % D]) {
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = 0;
  }
  st_words8(P + 8 * p, w);
}

void recv_chunks(size_t ndealers, size_t npad, size_t N, size_t L, const uint32_t* C, const uint32_t* xs, size_t m0,
                 size_t Ms, uint32_t* Q, uint32_t* R, hipStream_t stream) {
  if (!ndealers || !Ms || !N || !L) return;
  const size_t G = (N + L - 1) / L;
  hipLaunchKernelGGL(k_recv_chunks, dim3((unsigned)(npad / 64), (unsigned)G, (unsigned)Ms), dim3(64), 0, stream,
                     ndealers, npad, N, L, G, C, xs, m0, Q, R);
}

void recv_fold(size_t ndealers, size_t npad, size_t Gin, size_t r, const uint32_t* in, const uint32_t* digits,
               size_t dstride, size_t m0, size_t Ms, uint32_t* out, uint32_t* R, hipStream_t stream) {
  if (!ndealers || !Ms || Gin < 2 || r < 2) return;
  const size_t Gout = (Gin + r - 1) / r;
  hipLaunchKernelGGL(k_recv_fold, dim3((unsigned)(npad / 64), (unsigned)Gout, (unsigned)Ms), dim3(64), 0, stream,
                     ndealers, npad, Gin, r, in, digits, dstride, m0, out, R);
}

void pair_eval(size_t cnt, const uint32_t* list, const uint32_t* xs, const uint32_t* crow, const uint32_t* slot,
               const uint32_t* Eext, size_t stride, size_t N, uint32_t L, uint32_t G, uint32_t S,
               const uint32_t* digits, uint32_t* R, hipStream_t stream) {
  if (!cnt || !N || !L || G < 1 || G > 64 || (size_t)L * G < N || (1u << S) < G) return;
  hipLaunchKernelGGL(k_pair_eval, dim3((unsigned)cnt), dim3(64), 0, stream, list, xs, crow, slot, Eext, stride, N, L, G,
                     S, digits, R);
}

void seat_horner(size_t waves, size_t n, size_t N, size_t cols, uint32_t width, const uint32_t* wdesc,
                 const uint32_t* wseat, const uint32_t* scol, const uint32_t* C, uint32_t* R, hipStream_t stream) {
  const int wshift = seat_wshift(width);
  if (!waves || !n || !N || wshift < 0 || cols < n) return;
  hipLaunchKernelGGL(k_seat_horner, dim3((unsigned)waves), dim3(64), 0, stream, n, N, cols, (uint32_t)wshift,
                     wdesc, wseat, scol, C, R);
}

void seat_chunks(size_t waves, size_t n, size_t N, size_t cols, uint32_t width, size_t L, const uint32_t* wdesc,
                 const uint32_t* wseat, const uint32_t* scol, const uint32_t* C, uint32_t* Q, hipStream_t stream) {
  const int wshift = seat_wshift(width);
  if (!waves || !n || !N || !L || wshift < 0 || cols < n) return;
  const size_t G = (N + L - 1) / L;
  if (G > 65535) return;  // grid.y
  hipLaunchKernelGGL(k_seat_chunks, dim3((unsigned)waves, (unsigned)G), dim3(64), 0, stream, n, N, cols,
                     (uint32_t)wshift, L, wdesc, wseat, scol, C, Q);
}

void seat_fold(size_t waves, size_t n, uint32_t width, size_t Gin, const uint32_t* wdesc, const uint32_t* wseat,
               const uint32_t* xslot, const uint32_t* digits, size_t dstride, const uint32_t* in, uint32_t* out,
               uint32_t* R, hipStream_t stream) {
  const int wshift = seat_wshift(width);
  if (!waves || !n || Gin < 2 || Gin > 65535 || wshift < 0) return;
  hipLaunchKernelGGL(k_seat_fold, dim3((unsigned)waves, (unsigned)((Gin + 1) / 2)), dim3(64), 0, stream, n,
                     (uint32_t)wshift, Gin, wdesc, wseat, xslot, digits, dstride, in, out, R);
}

void seat_ok(size_t S, size_t n, const uint32_t* scol, const uint8_t* dok, const uint8_t* extra, uint8_t* sok,
             hipStream_t stream) {
  if (!S || !n) return;
  hipLaunchKernelGGL(k_seat_ok, dim3((unsigned)((S * n + 255) / 256)), dim3(256), 0, stream, S, n, scol, dok, extra,
                     sok);
}

void seat_decide(size_t S, size_t n, int round, const uint32_t* sx, const uint32_t* scer, const uint8_t* sok,
                 const uint8_t* qualified, uint8_t* dec, hipStream_t stream) {
  if (!S || !n) return;
  hipLaunchKernelGGL(k_seat_decide, dim3((unsigned)((S * n + 255) / 256)), dim3(256), 0, stream, S, n, round, sx, scer,
                     sok, qualified, dec);
}

void pair_ok(size_t cnt, const uint32_t* crow, const uint8_t* rowok, uint8_t* ok, hipStream_t stream) {
  if (!cnt) return;
  hipLaunchKernelGGL(k_pair_ok, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, stream, cnt, crow, rowok, ok);
}

void recv_decide(size_t M, size_t n, int round, const uint32_t* xs, const uint8_t* dok, const uint8_t* qualified,
                 uint8_t* dec, hipStream_t stream) {
  if (!M || !n) return;
  hipLaunchKernelGGL(k_recv_decide, dim3((unsigned)((M * n + 255) / 256)), dim3(256), 0, stream, M, n, round, xs, dok,
                     qualified, dec);
}

void recv_encode(size_t M, size_t D, const uint32_t* R, const uint8_t* dok, uint32_t* P, hipStream_t stream) {
  if (!M || !D) return;
  hipLaunchKernelGGL(k_recv_encode, dim3((unsigned)((M * D + 255) / 256)), dim3(256), 0, stream, M, D, R, dok, P);
}

}  // namespace dkgk
