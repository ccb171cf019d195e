// Round 1 of an operator's hosted seats on gfx950: K = pk * r for a dealing seat.
// A seat encrypts to each recipient key exactly twice -- the randomness s' and the share s, each under
// its own r (committee.rs:164-178, elgamal.rs:138-140) -- so a comb of the key (hybrid_batch.hip: 80 KiB
// written and read once, ~640 point operations for two products) never repays its build.  The two
// products share the base instead: one lane per key slot (seat p, recipient q) walks the signed radix-4
// digits of both scalars right to left (seat_deal.h) over M = 4^w pk,
//     2M by one doubling; K_0 += d_0 M, K_1 += d_1 M; M <- 2 (2M),
// 2 doublings and 2 complete additions per window, 128 windows, no table.  The addend of a digit is
// chosen among M, 2M and the identity (1, 1, 2, 0) by an LDS offset and selects, its sign as
// ge_add_signed applies it: every lane takes one code path whatever its digits (scalars and bases differ
// per lane, so a skipped addition would save nothing in a wave).  The additions are the complete formulas, so the
// identity key, small and large multiples of g and r = 0 need no special case.
// The cached forms of M and 2M (80 words) live in LDS, lane-interleaved as lds_put_cached lays them out
// (20 KiB per wave, each lane reads only its own column: no barrier); the two accumulators and M stay in
// VGPRs.  No scratch at 2 waves per SIMD.
#include "seat_deal.h"
#include "points.h"

namespace dkgk {

namespace {

// One field of the cached addend in this lane's LDS column (q = its limb 0), or of the identity's cached
// form (limb 0 = id0, the rest 0) where zero.  The opaque use keeps the loads inside the chain loop, as
// lds_get_fe's does.
DKG_DEV void seat_get_fe(fe& r, const uint32_t* q, bool zero, uint32_t id0) {
#pragma unroll
  for (int i = 0; i < 10; i++) {
    const uint32_t v = q[i * 64];
    r.v[i] = zero ? (i == 0 ? id0 : 0u) : v;
  }
  asm volatile("" : "+v"(r.v[0]), "+v"(r.v[1]), "+v"(r.v[2]), "+v"(r.v[3]), "+v"(r.v[4]), "+v"(r.v[5]),
               "+v"(r.v[6]), "+v"(r.v[7]), "+v"(r.v[8]), "+v"(r.v[9]));
}

// p = p + Q (neg = false) or p - Q (neg = true), Q the cached point at q or, where zero, the identity
// (1, 1, 2, 0): ge_add_signed term for term with the same operand order and bounds, neg and zero per
// lane, Q's fields read when the formula needs them (a whole addend in VGPRs next to two accumulators
// and M does not fit 256).
DKG_DEV void seat_add_lds(ge_p3& p, const uint32_t* q, bool neg, bool zero) {
  fe a, b, e, h, t, qv;
  fe_sub(t, p.Y, p.X);
  seat_get_fe(qv, q + (neg ? 0 : 10 * 64), zero, 1u);  // Y-X, or Y+X for -Q
  fe_mul(a, t, qv);
  fe_add(t, p.Y, p.X);
  seat_get_fe(qv, q + (neg ? 10 * 64 : 0), zero, 1u);
  fe_mul(b, t, qv);
  fe_sub(e, b, a);
  fe_add(h, b, a);
  seat_get_fe(qv, q + 30 * 64, zero, 0u);
  fe_mul(a, p.T, qv);       // c  (the term whose sign flips with Q)
  seat_get_fe(qv, q + 20 * 64, zero, 2u);
  fe_mul(b, p.Z, qv);       // d
  fe_neg(qv, a);            // -c = 2p - c <= 2p limbwise: a valid fe_sub subtrahend as is
  fe_cmov(a, qv, neg);      // a = +/-c (limbs <= 2^27)
  fe_sub(t, b, a);          // f = d - (+/-c) <= 1.5*2^27
  fe_add(b, b, a);          // g <= 2^27
  fe_mul(p.X, e, t);
  fe_mul(p.Y, b, h);
  fe_mul(p.Z, b, t);
  fe_mul(p.T, e, h);
}

}  // namespace

__global__ __launch_bounds__(64, 2) void k_seat_enc_mul(size_t slots, size_t n, const uint32_t* __restrict__ kbase,
                                                        const uint32_t* __restrict__ r,
                                                        const uint32_t* __restrict__ pk_ext, size_t stride,
                                                        uint32_t* __restrict__ K_ext, size_t count) {
  __shared__ uint32_t qs[2 * PT_WORDS * 64];  // cached M, then cached 2M
  const size_t slot = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (slot >= slots) return;
  uint32_t* qcol = qs + threadIdx.x;
  const uint32_t* rs = r + 16 * slot;  // the two scalars: words 0..7 of w = 0, then of w = 1
  ge_p3 m, acc0, acc1;
  pt_load(m, pk_ext, stride, (size_t)kbase[slot / n] + slot % n);
  ge_identity(acc0);
  ge_identity(acc1);
  int c0 = 0, c1 = 0;
  // acc += d * M for d in [-2, 2], the addend read from this lane's LDS column
  auto add_digit = [&](ge_p3& acc, int d) {
    const bool neg = d < 0, zero = d == 0;
    const uint32_t* src = qcol + (((neg ? -d : d) == 2) ? PT_WORDS * 64 : 0);
    seat_add_lds(acc, src, neg, zero);
  };
#pragma unroll 1
  for (int wi = 0; wi < SEAT_ENC_WINDOWS / 16; wi++) {
    // one word of each scalar per 16 windows, reread from memory: 16 VGPRs less than the scalars held
    const uint32_t w0 = rs[wi], w1 = rs[8 + wi];
#pragma unroll 1
    for (int win = 16 * wi; win < 16 * wi + 16; win++) {
      const int d0 = seat_enc_digit(seat_enc_bits(w0, win), win, c0);
      const int d1 = seat_enc_digit(seat_enc_bits(w1, win), win, c1);
      {
        ge_cached c;
        ge_to_cached(c, m);
        lds_put_cached(qcol, c);
        ge_dbl_lean<true>(m, m, true);  // 2M: T for its cached form
        ge_to_cached(c, m);
        lds_put_cached(qcol + PT_WORDS * 64, c);
      }
      add_digit(acc0, d0);
      add_digit(acc1, d1);
      if (win + 1 < SEAT_ENC_WINDOWS) ge_dbl_lean<true>(m, m, true);  // M of the next window (T: cached there)
    }
  }
  pt_store(K_ext, count, 2 * slot, acc0);
  pt_store(K_ext, count, 2 * slot + 1, acc1);
}

__global__ __launch_bounds__(256) void k_seat_key_index(size_t slots, size_t n, const uint32_t* __restrict__ kbase,
                                                        uint32_t* __restrict__ idx) {
  const size_t slot = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot < slots) idx[slot] = kbase[slot / n] + (uint32_t)(slot % n);
}

void seat_enc_mul(size_t slots, size_t n, const uint32_t* kbase, const uint32_t* r, const uint32_t* pk_ext,
                  size_t stride, uint32_t* K_ext, size_t count, hipStream_t stream) {
  if (!slots || !n) return;
  hipLaunchKernelGGL(k_seat_enc_mul, dim3((unsigned)((slots + 63) / 64)), dim3(64), 0, stream, slots, n, kbase, r,
                     pk_ext, stride, K_ext, count);
}

void seat_key_index(size_t slots, size_t n, const uint32_t* kbase, uint32_t* idx, hipStream_t stream) {
  if (!slots || !n) return;
  hipLaunchKernelGGL(k_seat_key_index, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, stream, slots, n, kbase,
                     idx);
}

}  // namespace dkgk
