// Rounds 3 and 5 of an operator's hosted seats on gfx950: the sum of a seat's
// qualified shares (Phases<Phase2>::proceed, committee.rs:453-467) and the interpolations at zero of
// Phases<Phase5>::finalise (committee.rs:745-789, polynomial.rs:162-184), one 64-lane workgroup per
// seat.  For a reconstructed dealer the seat holds its own point and the points the other final
// parties disclosed; lane a takes points a, a + 64, .. and computes
//   lambda_a = prod_{b != a} x_b / (x_b - x_a)
// from two chains of small multiplications (the x are party indices below 2^24; the denominator's
// factors are taken as magnitudes with the sign kept apart) and ONE inversion per point, the power
// den^(l - 2) in Montgomery form.  The lanes add y_a lambda_a into a running sum of their own over all
// points and all dealers; one shuffle reduction at the end leaves the seat's sum in lane 0.  Scalars are
// exact mod l, so the order of the additions does not show in the result.
#include "seat_finalise.h"
#include "sc25519.h"

namespace dkgk {

namespace {

constexpr int PT_WORDS = 40;  // one extended point (points.h)

DKG_DEV void sc_ld(sc& r, const uint32_t* __restrict__ p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1];
  r.v[0] = a.x, r.v[1] = a.y, r.v[2] = a.z, r.v[3] = a.w;
  r.v[4] = b.x, r.v[5] = b.y, r.v[6] = b.z, r.v[7] = b.w;
}

DKG_DEV void sc_st(uint32_t* __restrict__ p, const sc& s) {
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(s.v[0], s.v[1], s.v[2], s.v[3]);
  q[1] = make_uint4(s.v[4], s.v[5], s.v[6], s.v[7]);
}

// The sum of acc over the wave's 64 lanes, valid in lane 0 (the upper lanes hold partial sums).
DKG_DEV void sc_wave_sum(sc& acc) {
#pragma unroll 1
  for (int off = 32; off > 0; off >>= 1) {
    sc o;
#pragma unroll
    for (int w = 0; w < 8; w++) o.v[w] = (uint32_t)__shfl_down((int)acc.v[w], off, 64);
    sc_add(acc, acc, o);
  }
}

}  // namespace

__global__ __launch_bounds__(64) void k_seat_share_sum(size_t n, const uint32_t* __restrict__ scer,
                                                       const uint8_t* __restrict__ qualified,
                                                       const uint32_t* __restrict__ s, uint32_t* __restrict__ fs) {
  const size_t p = blockIdx.x;
  const uint8_t* q = qualified + (size_t)scer[p] * n;
  sc acc, x;
  sc_zero(acc);
  for (size_t i = threadIdx.x; i < n; i += 64) {
    if (!q[i]) continue;
    sc_ld(x, s + 8 * (p * n + i));
    sc_add(acc, acc, x);
  }
  sc_wave_sum(acc);
  if (threadIdx.x == 0) sc_st(fs + 8 * p, acc);
}

__global__ __launch_bounds__(64) void k_seat_lagrange(size_t n, const uint32_t* __restrict__ sslot,
                                                      const uint32_t* __restrict__ sx,
                                                      const uint8_t* __restrict__ skip,
                                                      const uint32_t* __restrict__ rptr,
                                                      const uint32_t* __restrict__ rdeal,
                                                      const uint32_t* __restrict__ dptr,
                                                      const uint32_t* __restrict__ dx,
                                                      const uint32_t* __restrict__ dy,
                                                      const uint32_t* __restrict__ s, uint32_t max_points,
                                                      uint32_t* __restrict__ sigma) {
  extern __shared__ uint32_t lds[];  // xs [max_points], then ysrc [max_points]
  uint32_t* xs = lds;
  uint32_t* ysrc = lds + max_points;
  const size_t p = blockIdx.x;
  const int lane = threadIdx.x;
  sc acc;
  sc_zero(acc);
  if (skip[p]) {  // block-uniform
    if (lane == 0) sc_st(sigma + 8 * p, acc);
    return;
  }
  const uint32_t x0 = sx[p], slot = sslot[p];
  sc rr, zero;
  sc_zero(zero);
#pragma unroll
  for (int i = 0; i < 8; i++) rr.v[i] = sc_const::RR[i];
  for (uint32_t k = rptr[slot]; k < rptr[slot + 1]; k++) {
    const uint32_t e0 = dptr[k], len = dptr[k + 1] - e0;
    // the point list: the seat's own first, then the disclosures in list order without the seat's own
    // sender (at most one: the senders of a record are distinct)
    uint32_t self = 0xffffffffu;
    for (uint32_t e = lane; e < len; e += 64)
      if (dx[e0 + e] == x0) self = e;
#pragma unroll 1
    for (int off = 32; off > 0; off >>= 1) {
      const uint32_t o = (uint32_t)__shfl_xor((int)self, off, 64);
      self = o < self ? o : self;
    }
    uint32_t m = 1 + len - (self != 0xffffffffu ? 1u : 0u);
    if (m > max_points) m = max_points;  // never taken: the host sizes max_points by the longest record
    __syncthreads();  // the previous dealer's reads of the list are over
    if (lane == 0) {
      xs[0] = x0;
      ysrc[0] = 0xffffffffu;
    }
    for (uint32_t e = lane; e < len; e += 64) {
      if (e == self) continue;
      const uint32_t pos = 1 + e - (self != 0xffffffffu && e > self ? 1u : 0u);
      if (pos >= m) continue;
      xs[pos] = dx[e0 + e];
      ysrc[pos] = e0 + e;
    }
    __syncthreads();
    for (uint32_t a = lane; a < m; a += 64) {
      const uint32_t xa = xs[a];
      sc num, den;
      sc_zero(num);
      num.v[0] = 1;
      den = num;
      uint32_t negs = 0;
      for (uint32_t b = 0; b < m; b++) {
        if (b == a) continue;
        const uint32_t xb = xs[b];
        sc_mul_small_add(num, num, xb, zero);
        negs ^= xb < xa ? 1u : 0u;
        sc_mul_small_add(den, den, xb < xa ? xa - xb : xb - xa, zero);
      }
      sc t, y;
      sc_mont_mul(t, den, rr);  // den R
      sc_mont_inv(t, t);        // R / den
      sc_mont_mul(t, num, t);   // lambda_a up to the sign
      sc_mont_mul(t, t, rr);    // lambda_a R
      const uint32_t src = ysrc[a];
      sc_ld(y, src == 0xffffffffu ? s + 8 * (p * n + rdeal[k]) : dy + 8 * (size_t)src);
      sc_mont_mul(t, y, t);     // y_a lambda_a
      if (negs) sc_neg(t, t);
      sc_add(acc, acc, t);
    }
  }
  sc_wave_sum(acc);
  if (lane == 0) sc_st(sigma + 8 * p, acc);
}

__global__ __launch_bounds__(256) void k_seat_gather_pts(size_t count, const uint32_t* __restrict__ idx,
                                                         const uint32_t* __restrict__ src, size_t sstride,
                                                         uint32_t* __restrict__ dst, size_t dstride) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= count) return;
  const uint32_t e = idx[p];
  if (e == SEAT_ROW_NONE) return;
#pragma unroll 8
  for (int w = 0; w < PT_WORDS; w++) dst[w * dstride + p] = src[w * sstride + e];
}

void seat_share_sum(size_t S, size_t n, const uint32_t* scer, const uint8_t* qualified, const uint32_t* s,
                    uint32_t* fs, hipStream_t stream) {
  if (!S || !n) return;
  hipLaunchKernelGGL(k_seat_share_sum, dim3((unsigned)S), dim3(64), 0, stream, n, scer, qualified, s, fs);
}

void seat_lagrange(size_t S, size_t n, const uint32_t* sslot, const uint32_t* sx, const uint8_t* skip,
                   const uint32_t* rptr, const uint32_t* rdeal, const uint32_t* dptr, const uint32_t* dx,
                   const uint32_t* dy, const uint32_t* s, size_t max_points, uint32_t* sigma, hipStream_t stream) {
  if (!S || !n || !max_points || max_points > SEAT_LAGRANGE_MAX_POINTS) return;
  hipLaunchKernelGGL(k_seat_lagrange, dim3((unsigned)S), dim3(64), 8 * max_points, stream, n, sslot, sx, skip, rptr,
                     rdeal, dptr, dx, dy, s, (uint32_t)max_points, sigma);
}

void seat_gather_points(size_t count, const uint32_t* idx, const uint32_t* src, size_t sstride, uint32_t* dst,
                        size_t dstride, hipStream_t stream) {
  if (!count) return;
  hipLaunchKernelGGL(k_seat_gather_pts, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, count, idx, src,
                     sstride, dst, dstride);
}

}  // namespace dkgk
