// Complaints on gfx950.  Round 2: ProofOfMisbehaviour::generate (broadcast.rs:189-226) and
// MisbehavingPartiesRound1::verify (broadcast.rs:50-99 with ProofOfMisbehaviour::verify, :227-283) as
// batches, one work item per complaint.  A proof is (share_key, randomness_key, c1, r1, c2, r2): the
// two recovered symmetric keys K = sk * e1 and a DLEQ(g, e1, pk, K; sk) proof for each
// (correct_hybrid_decryption_key/zkp.rs:27-47, dl_equality/zkp.rs:29-74).  The work is staged as in
// hybrid.hip, so that no kernel carries both a scalar-multiplication loop and the ARX state:
//   prep    : scalars (reductions, negations), the points to decode, SymmetricKey::process (ARX);
//   ladder  : the variable-base products (k_cmp_ladder), one item per product;
//   combs   : the g / h terms through the shared fixed-base kernels (fixed_base);
//   horner  : P_i(j) per (accused, accuser) pair (k_cmp_horner), or the difference tables (runtime);
//   check   : the two check elements h p1 + g p2, h p2 + g p1 against P_i(j) (k_cv_check, combs);
//   final   : the Fiat-Shamir challenges (two-block Blake2b) and the verdict (ARX).
// Round 4: MisbehavingPartiesRound3::verify (broadcast.rs:104-144) as a batch, one lane per complaint
// (k_c3_prep / k_c3_check / k_c3_final at the end of this file): no proofs, so only the horner / tables
// stage and a check of both sides from one walk of the g comb.
#include "kernels.h"
#include "points.h"
#include "hybrid_dev.h"
#include "sym.h"

namespace dkgk {

namespace {

// the Ristretto basepoint's encoding as little-endian words (ChallengeContext's first base)
__device__ const uint32_t CMP_G[8] = {0x0aaef2e2u, 0x714ebc6au, 0x61a984a8u, 0x5f5100c5u,
                                      0x6a0be358u, 0x8ddd82a5u, 0x4559a6b6u, 0x762d8de0u};

// Scalar::from_bytes_mod_order_wide of a 64-byte hash: lo + hi 2^256 mod l
DKG_DEV void sc_wide(sc& r, const uint64_t (&h)[8]) {
  uint32_t lo[8], hi[8];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    lo[2 * i] = (uint32_t)h[i];
    lo[2 * i + 1] = (uint32_t)(h[i] >> 32);
    hi[2 * i] = (uint32_t)h[4 + i];
    hi[2 * i + 1] = (uint32_t)(h[4 + i] >> 32);
  }
  sc a, b, rr;
  sc_reduce256(a, lo);
  sc_reduce256(b, hi);
#pragma unroll
  for (int i = 0; i < 8; i++) rr.v[i] = sc_const::RR[i];
  sc_mont_mul(b, b, rr);  // hi * 2^256
  sc_add(r, a, b);
}

// Scalar::hash_from_bytes::<Blake2b> (groups.rs:50-52) of ChallengeContext g || e1 || pk || K || a1 || a2
// (challenge_context.rs:14-41); every part 8 words
DKG_DEV void dleq_challenge(sc& c, const uint32_t* e1, const uint32_t* pk, const uint32_t* K, const uint32_t* a1,
                            const uint32_t* a2) {
  uint64_t m[32];
  const uint32_t* parts[6] = {CMP_G, e1, pk, K, a1, a2};
#pragma unroll
  for (int p = 0; p < 6; p++)
#pragma unroll
    for (int j = 0; j < 4; j++) m[4 * p + j] = (uint64_t)parts[p][2 * j] | ((uint64_t)parts[p][2 * j + 1] << 32);
#pragma unroll
  for (int j = 24; j < 32; j++) m[j] = 0;
  uint64_t h[8];
  sym::blake2b_2block(h, m, 192, 64);
  sc_wide(c, h);
}

// SymmetricKey::process + Scalar::from_bytes (from_bits, reduced) of a 32-byte ciphertext
// (elgamal.rs:172-193; as k_sym_xor's decrypt branch)
DKG_DEV void sym_scalar(sc& r, const uint32_t* K, const uint32_t* ct) {
  uint64_t m[16];
#pragma unroll
  for (int j = 0; j < 4; j++) m[j] = (uint64_t)K[2 * j] | ((uint64_t)K[2 * j + 1] << 32);
#pragma unroll
  for (int j = 4; j < 16; j++) m[j] = 0;
  uint64_t h[8];
  sym::blake2b_1block(h, m, 32, 64);
  uint32_t key[8], nonce[3];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    key[2 * j] = (uint32_t)h[j];
    key[2 * j + 1] = (uint32_t)(h[j] >> 32);
  }
  nonce[0] = (uint32_t)h[4];
  nonce[1] = (uint32_t)(h[4] >> 32);
  nonce[2] = (uint32_t)h[5];
  uint32_t ks[16];
  sym::chacha20_ietf_block(ks, key, 0u, nonce);
  uint32_t v[8];
#pragma unroll
  for (int j = 0; j < 8; j++) v[j] = ct[j] ^ ks[j];
  v[7] &= 0x7fffffffu;
  sc_reduce256(r, v);
}

DKG_DEV void copy8(uint32_t* dst, const uint32_t* src) {
#pragma unroll
  for (int j = 0; j < 8; j++) dst[j] = src[j];
}
DKG_DEV void sc_load_reduced(sc& r, const uint32_t* p) {
  uint32_t w[8];
#pragma unroll
  for (int j = 0; j < 8; j++) w[j] = p[j];
  w[7] &= 0x7fffffffu;  // from_bits, as k_reduce_scalars
  sc_reduce256(r, w);
}
DKG_DEV void sc_store(uint32_t* p, const sc& s) {
#pragma unroll
  for (int j = 0; j < 8; j++) p[j] = s.v[j];
}
DKG_DEV bool eq8(const uint32_t* a, const uint32_t* b) {
  uint32_t d = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) d |= a[j] ^ b[j];
  return d == 0;
}

// bits [bit, bit + 2) of s; `bit` is wave-uniform (select chain, no indexed register file access)
DKG_DEV uint32_t sc_bits2(const sc& s, int bit) {
  const int wi = bit >> 5;
  uint32_t word = s.v[0];
#pragma unroll
  for (int k = 1; k < 8; k++) word = (wi == k) ? s.v[k] : word;
  return (word >> (bit & 31)) & 3u;  // bit is even in the window walk, so a window never straddles words
}

}  // namespace

// ------------------------------------------------------------------ variable-base products
// One item per product.  joint: out = a P + b Q by Straus' interleaving, one doubling per bit and the
// addend (a_bit + 2 b_bit) in {P, Q, P + Q}.  Single base (joint = 0): out = a P with width-2
// windows, which is the same walk over the bases (P, 2P): two doublings per step and the addend in
// {P, 2P, 3P} -- 127 additions for 253 doublings.  (Two products of one base that shared their
// doublings right-to-left would pay an addition slot per bit and scalar -- 253 doublings + 506
// slots -- which is more field products than two windowed walks, 506 + 254.)  Scalars canonical.
// Lanes carry independent scalars, so the walk is branch-free: every lane adds at every step, the
// zero digit adding the identity.  The three addends (cached form) sit in a global table T laid out
// [3][40 words][items, padded to 64]; the step's addend goes through the wave's LDS slot so that the
// chain keeps one point in VGPRs, as k_dec_mul_w4 (whose launch bounds these are).
__global__ __launch_bounds__(64, DKG_DEC_W4_WAVES) void k_cmp_ladder(size_t cnt, int joint, const uint32_t* __restrict__ bp,
                                                      const uint32_t* __restrict__ bq,
                                                      const uint32_t* __restrict__ sa,
                                                      const uint32_t* __restrict__ sb,
                                                      const uint32_t* __restrict__ Pext, size_t pstride,
                                                      uint32_t* __restrict__ T, uint32_t* __restrict__ out) {
  __shared__ uint32_t qs[PT_WORDS * 64];
  uint32_t* qcol = qs + threadIdx.x;
  const size_t k = (size_t)blockIdx.x * 64 + threadIdx.x;
  const bool live = k < cnt;
  const size_t kk = live ? k : 0;
  const size_t stride = (size_t)gridDim.x * 64;
  uint32_t* tb = T + k;  // padded: every lane of the grid owns a column
  ge_p3 x;
  {
    ge_p3 q;
    ge_cached c;
    pt_load(x, Pext, pstride, bp[kk]);
    ge_to_cached(c, x);
    lds_put_cached(tb, c, (int)stride);
    if (joint) pt_load(q, Pext, pstride, bq[kk]);
    else ge_dbl<true>(q, x);
    ge_to_cached(c, q);
    lds_put_cached(tb + PT_WORDS * stride, c, (int)stride);
    ge_add(x, x, c);
    ge_to_cached(c, x);
    lds_put_cached(tb + 2 * PT_WORDS * stride, c, (int)stride);
  }
  sc a, b;
  sc_load(a, sa + 8 * kk);
  if (joint) sc_load(b, sb + 8 * kk);
  else sc_zero(b);
  ge_identity(x);
  const int steps = joint ? 253 : 127;
#pragma unroll 1
  for (int s = steps - 1; s >= 0; s--) {
    uint32_t d;
    if (joint) {
      d = (sc_bits2(a, s) & 1u) | ((sc_bits2(b, s) & 1u) << 1);
    } else {
      d = sc_bits2(a, 2 * s);
      ge_dbl_lean<DKG_DEC_IL != 0>(x, x, false);
    }
    ge_dbl_lean<DKG_DEC_IL != 0>(x, x, true);
    if (__builtin_amdgcn_ballot_w64(d != 0) == 0) continue;  // no lane of the wave adds
    const uint32_t* src = tb + (size_t)(d ? d - 1 : 0) * PT_WORDS * stride;
#pragma unroll
    for (int w = 0; w < PT_WORDS; w++) {
      const uint32_t idw = (w == 0 || w == 10) ? 1u : (w == 20 ? 2u : 0u);  // cached identity (1, 1, 2, 0)
      const uint32_t v = src[(size_t)w * stride];
      qcol[w * 64] = d ? v : idw;
    }
    ge_add_lds<DKG_DEC_IL != 0>(x, x, qcol, false, 64, s == 0);
  }
  if (live) pt_store(out, cnt, k, x);
}

size_t cmp_ladder_table_words(size_t cnt) { return 3 * (size_t)PT_WORDS * ((cnt + 63) / 64 * 64); }

void cmp_ladder(size_t cnt, bool joint, const uint32_t* bp, const uint32_t* bq, const uint32_t* sa, const uint32_t* sb,
                const uint32_t* Pext, size_t pstride, uint32_t* T, uint32_t* out, hipStream_t stream) {
  if (!cnt) return;
  hipLaunchKernelGGL(k_cmp_ladder, dim3((unsigned)((cnt + 63) / 64)), dim3(64), 0, stream, cnt, joint ? 1 : 0, bp, bq,
                     sa, sb, Pext, pstride, T, out);
}

// ------------------------------------------------------------------ P_i(j) per pair
// Horner in the exponent, k_horner generalised to a list of (row, index) pairs: lane = pair
// list[k] = complaint c, row = crow[c] - 1 of the decoded commitments Eext (element row * N + k),
// index x = xs[c] (< 2^nb).  The commitment row is its own array, apart from the evaluation index:
// one ceremony passes (accuser, accused); a batch passes the accuser within its ceremony and the
// accused's row among the gathered rows (k_gather_rows), so lanes of one wave may walk rows of
// different ceremonies.  The indices differ between lanes, so x * acc is a branch-free
// double-and-add over nb bits (a bit no lane of the wave has set skips its addition).  R: point-major
// [c][40].
__global__ __launch_bounds__(64, 2) void k_cmp_horner(size_t cnt, const uint32_t* __restrict__ list,
                                                      const uint32_t* __restrict__ xs,
                                                      const uint32_t* __restrict__ crow,
                                                      const uint32_t* __restrict__ Eext, size_t stride, size_t N, int nb,
                                                      uint32_t* __restrict__ R) {
  const size_t k = (size_t)blockIdx.x * 64 + threadIdx.x;
  const bool live = k < cnt;
  const size_t c = list[live ? k : 0];
  const uint32_t x = xs[c];
  const size_t row = (size_t)(crow[c] - 1) * N;
  ge_p3 acc;
  pt_load(acc, Eext, stride, row + N - 1);
#pragma unroll 1
  for (size_t kk = N - 1; kk-- > 0;) {
    ge_cached bc;
    ge_to_cached(bc, acc);
    ge_identity(acc);
#pragma unroll 1
    for (int b = nb - 1; b >= 0; b--) {
      ge_dbl_lean(acc, acc, true);
      const bool bit = (x >> b) & 1u;
      if (__builtin_amdgcn_ballot_w64(bit) == 0) continue;
      ge_p3 sum;
      ge_add(sum, acc, bc);
#pragma unroll
      for (int w = 0; w < PT_WORDS; w++) pt_word(acc, w) = bit ? pt_word(sum, w) : pt_word(acc, w);
    }
    ge_p3 e;
    pt_load(e, Eext, stride, row + kk);
    ge_to_cached(bc, e);
    ge_add(acc, acc, bc);
  }
  if (live) pt_store_aos(R, c, acc);
}

void cmp_horner(size_t cnt, const uint32_t* list, const uint32_t* xs, const uint32_t* crow, const uint32_t* Eext,
                size_t stride, size_t N, int nb, uint32_t* R, hipStream_t stream) {
  if (!cnt) return;
  hipLaunchKernelGGL(k_cmp_horner, dim3((unsigned)((cnt + 63) / 64)), dim3(64), 0, stream, cnt, list, xs, crow,
                     Eext, stride, N, nb, R);
}

// ------------------------------------------------------------------ verify: prep / check / final
// Thread (c, m): proof m of complaint c (m = 0 the share's, m = 1 the randomness's).  enc [C][32 words]
// = e1_rand | ct_rand | e1_share | ct_share, proofs [C][48 words] = K_share | K_rand | c1 | r1 | c2 | r2.
// Out: the points to decode Pc [5C][8] (pk_accuser, e1_share, K_share, e1_rand, K_rand), the
// responses rs [2C][8] and negated challenges nc [2C][8] (canonical), the decrypted scalars p12
// [2C][8] (p1 = share, p2 = randomness), and the ladders' base indices.  party [C]: the accuser's
// 1-based slot in pk -- the accuser itself for one ceremony, g n + accuser in a batch of [B][n] keys.
__global__ __launch_bounds__(256) void k_cv_prep(size_t C, const uint32_t* __restrict__ party,
                                                 const uint32_t* __restrict__ pk, const uint32_t* __restrict__ enc,
                                                 const uint32_t* __restrict__ proofs, uint32_t* __restrict__ Pc,
                                                 uint32_t* __restrict__ rs, uint32_t* __restrict__ nc,
                                                 uint32_t* __restrict__ p12, uint32_t* __restrict__ bp1,
                                                 uint32_t* __restrict__ bp2, uint32_t* __restrict__ bq2) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 2 * C) return;
  const size_t c = idx >> 1, m = idx & 1;
  const uint32_t* e = enc + 32 * c;
  const uint32_t* P = proofs + 48 * c;
  const uint32_t* e1 = e + (m ? 0 : 16);
  const uint32_t* ct = e + (m ? 8 : 24);
  const uint32_t* K = P + 8 * m;
  if (m == 0) copy8(Pc + 8 * (5 * c), pk + 8 * (size_t)(party[c] - 1));
  copy8(Pc + 8 * (5 * c + 1 + 2 * m), e1);
  copy8(Pc + 8 * (5 * c + 2 + 2 * m), K);
  sc x, y;
  sc_load_reduced(x, P + 16 + 16 * m);  // challenge
  sc_neg(y, x);
  sc_store(nc + 8 * idx, y);
  sc_load_reduced(x, P + 24 + 16 * m);  // response
  sc_store(rs + 8 * idx, x);
  sym_scalar(x, K, ct);
  sc_store(p12 + 8 * idx, x);
  bp1[idx] = (uint32_t)(5 * c);
  bp2[idx] = (uint32_t)(5 * c + 1 + 2 * m);
  bq2[idx] = (uint32_t)(5 * c + 2 + 2 * m);
}

void cv_prep(size_t C, const uint32_t* party, const uint32_t* pk, const uint32_t* enc, const uint32_t* proofs,
             uint32_t* Pc, uint32_t* rs, uint32_t* nc, uint32_t* p12, uint32_t* bp1, uint32_t* bp2, uint32_t* bq2,
             hipStream_t stream) {
  if (!C) return;
  hipLaunchKernelGGL(k_cv_prep, dim3((unsigned)((2 * C + 255) / 256)), dim3(256), 0, stream, C, party, pk, enc, proofs,
                     Pc, rs, nc, p12, bp1, bp2, bq2);
}

// The two check elements of complaint c against P = P_accused(accuser): eq[2c] = (h p1 + g p2 == P),
// the quirk of ProofOfMisbehaviour::verify (broadcast.rs:271-283), eq[2c + 1] = (h p2 + g p1 == P), the
// accusation (:87-96).  ridx[c]: bit 31 clear = element of Rh (k_cmp_horner, P itself); set = element
// of Rt, the difference tables' evaluations, which hold b_j P(j) when `scale` is given (b_j 2^256 mod
// l at scale + 8 (j - 1)): the scalars are then taken to b_j p first, as k_check does.  `accuser` is
// the evaluation index j within the ceremony (the scale slot), never a party or commitment row.
__global__ __launch_bounds__(256, DKG_COMB_WAVES) void k_cv_check(size_t C, const uint32_t* __restrict__ accuser,
                                                  const uint32_t* __restrict__ p12, const uint32_t* __restrict__ ridx,
                                                  const uint32_t* __restrict__ Rh, const uint32_t* __restrict__ Rt,
                                                  const uint32_t* __restrict__ scale,
                                                  const uint32_t* __restrict__ tab_g,
                                                  const uint32_t* __restrict__ tab_h, uint8_t* __restrict__ eq) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 2 * C) return;
  const size_t c = idx >> 1, m = idx & 1;  // m = 0 the quirk, 1 the accusation
  const uint32_t ri = ridx[c];
  const bool tab = ri >> 31;
  sc x, f;
  const bool scaled = tab && scale;
  if (scaled) sc_load(f, scale + 8 * (size_t)(accuser[c] - 1));
  ge_p3 acc, r;
  ge_identity(acc);
  sc_load(x, p12 + 8 * (2 * c + m));  // h * (p1 | p2)
  if (scaled) sc_mont_mul(x, x, f);
  combw_mul_add(acc, x, tab_h);
  sc_load(x, p12 + 8 * (2 * c + 1 - m));  // g * (p2 | p1)
  if (scaled) sc_mont_mul(x, x, f);
  combw_mul_add(acc, x, tab_g);
  pt_load_aos(r, tab ? Rt : Rh, ri & 0x7fffffffu);
  eq[idx] = ristretto_eq(acc, r) ? 1 : 0;
}

void cv_check(size_t C, const uint32_t* accuser, const uint32_t* p12, const uint32_t* ridx, const uint32_t* Rh,
              const uint32_t* Rt, const uint32_t* scale, const uint32_t* tab_g, const uint32_t* tab_h, uint8_t* eq,
              hipStream_t stream) {
  if (!C) return;
  hipLaunchKernelGGL(k_cv_check, dim3((unsigned)((2 * C + 255) / 256)), dim3(256), 0, stream, C, accuser, p12, ridx, Rh,
                     Rt, scale, tab_g, tab_h, eq);
}

// Verdict of complaint c (the codes of dkg_complaint1_verify, and 4 when the accused published no
// phase-1 broadcast, committee.rs:377-380).  a1c / a2c [2C][8]: the encoded announcements g r - pk c,
// e1 r - K c; pok [5C] decode flags of k_cv_prep's points.  party [C] as k_cv_prep's; crow [C]: the
// accused's 1-based commitment row, which indexes rowok (= the row decodes) and fetched (may be
// null) -- the accused itself for one ceremony, its gathered row in a batch.
__global__ __launch_bounds__(256) void k_cv_final(size_t C, const uint32_t* __restrict__ party,
                                                  const uint32_t* __restrict__ crow,
                                                  const uint32_t* __restrict__ pk, const uint32_t* __restrict__ enc,
                                                  const uint32_t* __restrict__ proofs,
                                                  const uint32_t* __restrict__ a1c, const uint32_t* __restrict__ a2c,
                                                  const uint8_t* __restrict__ pok, const uint8_t* __restrict__ rowok,
                                                  const uint8_t* __restrict__ fetched, const uint8_t* __restrict__ eq,
                                                  int32_t* __restrict__ verdict) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const size_t i = crow[c] - 1;
  const uint32_t* pkj = pk + 8 * (size_t)(party[c] - 1);
  bool valid = true;
#pragma unroll 1
  for (int m = 0; m < 2; m++) {
    sc ch;
    dleq_challenge(ch, enc + 32 * c + (m ? 0 : 16), pkj, proofs + 48 * c + 8 * m, a1c + 8 * (2 * c + m),
                   a2c + 8 * (2 * c + m));
    valid = valid && eq8(ch.v, proofs + 48 * c + 16 + 16 * m);  // the proof's challenge bytes as sent
  }
  bool dec = rowok[i] != 0;
#pragma unroll
  for (int p = 0; p < 5; p++) dec = dec && pok[5 * c + p];
  int32_t v;
  if (fetched && !fetched[i]) v = 4;
  else if (!dec) v = -1;
  else if (!valid) v = 1;        // InvalidProofOfMisbehaviour
  else if (eq[2 * c]) v = 1;     // ProofOfMisbehaviour::verify's check (:271-283)
  else if (eq[2 * c + 1]) v = 2; // FalseClaimedInequality (:94-96)
  else v = 0;
  verdict[c] = v;
}

void cv_final(size_t C, const uint32_t* party, const uint32_t* crow, const uint32_t* pk, const uint32_t* enc,
              const uint32_t* proofs, const uint32_t* a1c, const uint32_t* a2c, const uint8_t* pok, const uint8_t* rowok,
              const uint8_t* fetched, const uint8_t* eq, int32_t* verdict, hipStream_t stream) {
  if (!C) return;
  hipLaunchKernelGGL(k_cv_final, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, stream, C, party, crow, pk, enc,
                     proofs, a1c, a2c, pok, rowok, fetched, eq, verdict);
}

// ------------------------------------------------------------------ prove: prep / finish
// sk [C][8], enc [C][32], w [C][16] raw words.  Out: Pc [2C][8] = (e1_share, e1_rand); the ladders'
// scalars ls [4C][8] = (sk, sk, w1, w2) on bases lb [4C] = (e1_share, e1_rand, e1_share, e1_rand);
// the comb's scalars gs [3C][8] = (sk, w1, w2).
__global__ __launch_bounds__(256) void k_cp_prep(size_t C, const uint32_t* __restrict__ sk, const uint32_t* __restrict__ enc,
                                                 const uint32_t* __restrict__ w, uint32_t* __restrict__ Pc,
                                                 uint32_t* __restrict__ ls, uint32_t* __restrict__ lb,
                                                 uint32_t* __restrict__ gs) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  copy8(Pc + 8 * (2 * c), enc + 32 * c + 16);
  copy8(Pc + 8 * (2 * c + 1), enc + 32 * c);
  sc x;
  sc_load_reduced(x, sk + 8 * c);
  sc_store(ls + 8 * (4 * c), x);
  sc_store(ls + 8 * (4 * c + 1), x);
  sc_store(gs + 8 * (3 * c), x);
  sc_load_reduced(x, w + 16 * c);
  sc_store(ls + 8 * (4 * c + 2), x);
  sc_store(gs + 8 * (3 * c + 1), x);
  sc_load_reduced(x, w + 16 * c + 8);
  sc_store(ls + 8 * (4 * c + 3), x);
  sc_store(gs + 8 * (3 * c + 2), x);
#pragma unroll
  for (int k = 0; k < 4; k++) lb[4 * c + k] = (uint32_t)(2 * c + (k & 1));
}

void cp_prep(size_t C, const uint32_t* sk, const uint32_t* enc, const uint32_t* w, uint32_t* Pc, uint32_t* ls,
             uint32_t* lb, uint32_t* gs, hipStream_t stream) {
  if (!C) return;
  hipLaunchKernelGGL(k_cp_prep, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, stream, C, sk, enc, w, Pc, ls, lb, gs);
}

// lc [4C][8] = encodings of (K_share, K_rand, e1_share w1, e1_rand w2), gc [3C][8] of (pk, g w1, g w2),
// ls / gs as k_cp_prep: challenge c = H(g, e1, pk, K, g w, e1 w), response r = c sk + w
// (dl_equality/zkp.rs:29-49) -> proofs [C][48 words].
__global__ __launch_bounds__(256) void k_cp_finish(size_t C, const uint32_t* __restrict__ enc,
                                                   const uint32_t* __restrict__ lc, const uint32_t* __restrict__ gc,
                                                   const uint32_t* __restrict__ gs, uint32_t* __restrict__ proofs) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  uint32_t* P = proofs + 48 * c;
  copy8(P, lc + 8 * (4 * c));
  copy8(P + 8, lc + 8 * (4 * c + 1));
  sc x;
  sc_load(x, gs + 8 * (3 * c));
#pragma unroll 1
  for (int m = 0; m < 2; m++) {
    sc ch, wn, r;
    dleq_challenge(ch, enc + 32 * c + (m ? 0 : 16), gc + 8 * (3 * c), lc + 8 * (4 * c + m), gc + 8 * (3 * c + 1 + m),
                   lc + 8 * (4 * c + 2 + m));
    sc_load(wn, gs + 8 * (3 * c + 1 + m));
    sc_mul(r, ch, x);
    sc_add(r, r, wn);
    sc_store(P + 16 + 16 * m, ch);
    sc_store(P + 24 + 16 * m, r);
  }
}

void cp_finish(size_t C, const uint32_t* enc, const uint32_t* lc, const uint32_t* gc, const uint32_t* gs,
               uint32_t* proofs, hipStream_t stream) {
  if (!C) return;
  hipLaunchKernelGGL(k_cp_finish, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, stream, C, enc, lc, gc, gs, proofs);
}

// ------------------------------------------------------------------ the qualified set from proven complaints
// One wave per dealer row i of dec [rows][n]: qmask[i] = row i holds no MISSING and cmask[i] (no
// verified complaint against i, committee.rs:370-398); rej[i] = !qmask[i] for the host half.
__global__ __launch_bounds__(64) void k_qualified_complaints(size_t n, const uint8_t* __restrict__ dec,
                                                             const uint8_t* __restrict__ cmask,
                                                             uint8_t* __restrict__ rej, uint8_t* __restrict__ qmask) {
  const size_t i = blockIdx.x;
  bool missing = false;
  for (size_t j = threadIdx.x; j < n; j += 64) missing = missing || dec[i * n + j] == 4;
  const bool any = __builtin_amdgcn_ballot_w64(missing) != 0;
  if (threadIdx.x == 0) {
    const uint8_t q = (!any && cmask[i]) ? 1 : 0;
    qmask[i] = q;
    rej[i] = !q;
  }
}

void qualified_complaints(size_t rows, size_t n, const uint8_t* dec, const uint8_t* cmask, uint8_t* rej, uint8_t* qmask,
                          hipStream_t stream) {
  if (!rows) return;
  hipLaunchKernelGGL(k_qualified_complaints, dim3((unsigned)rows), dim3(64), 0, stream, n, dec, cmask, rej, qmask);
}

// ------------------------------------------------------------------ round-4 complaints: prep / check / final
// MisbehavingPartiesRound3::verify (broadcast.rs:104-144) for C complaints, lane = complaint.  A
// complaint discloses the accuser's decrypted pair; it holds when the pair passes against the
// accused's E row and fails against its A row.  Both rows live in ONE decoded array of 2 `arows` rows
// (E rows 0..arows-1, A rows arows..2 arows-1), so complaint c is the two evaluation items 2c = (row
// i, index j) and 2c + 1 = (row arows + i, index j) of k_cmp_horner / the difference tables.  One
// ceremony: arows = n and the rows i = crow[c] are the accused dealers; a batch: the arows gathered
// rows (k_gather_rows), crow[c] the accused's place among them.  j = accuser[c], the index within
// the ceremony.
// prep: share / randomness [C][8] raw -> sr [2C][8] canonical (k_reduce_scalars' reduction, what the
// host-driven primitive's upload applies), and the items' index lists acc2 / acd2 [2C].
__global__ __launch_bounds__(256) void k_c3_prep(size_t C, uint32_t arows, const uint32_t* __restrict__ accuser,
                                                 const uint32_t* __restrict__ crow,
                                                 const uint32_t* __restrict__ share,
                                                 const uint32_t* __restrict__ randomness, uint32_t* __restrict__ sr,
                                                 uint32_t* __restrict__ acc2, uint32_t* __restrict__ acd2) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  sc x;
  sc_load_reduced(x, share + 8 * c);
  sc_store(sr + 8 * (2 * c), x);
  sc_load_reduced(x, randomness + 8 * c);
  sc_store(sr + 8 * (2 * c + 1), x);
  acc2[2 * c] = acc2[2 * c + 1] = accuser[c];
  acd2[2 * c] = crow[c];
  acd2[2 * c + 1] = arows + crow[c];
}

void c3_prep(size_t C, size_t arows, const uint32_t* accuser, const uint32_t* crow, const uint32_t* share,
             const uint32_t* randomness, uint32_t* sr, uint32_t* acc2, uint32_t* acd2, hipStream_t stream) {
  if (!C) return;
  hipLaunchKernelGGL(k_c3_prep, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, stream, C, (uint32_t)arows, accuser,
                     crow, share, randomness, sr, acc2, acd2);
}

// eq[2c] = (g share + h randomness == P^E_i(j)), eq[2c + 1] = (g share == P^A_i(j)): one walk of the g
// comb serves both sides, the h comb's terms are added to it.  ridx [2C] per item as k_cv_check's
// (bit 31: Rt, the tables' b_j P(j) when `scale` is given); both items of a complaint take the same
// source, so the scalars are scaled once.  `accuser` is the evaluation index (the scale slot).
__global__ __launch_bounds__(256, DKG_COMB_WAVES) void k_c3_check(size_t C, const uint32_t* __restrict__ accuser,
                                                  const uint32_t* __restrict__ sr, const uint32_t* __restrict__ ridx,
                                                  const uint32_t* __restrict__ Rh, const uint32_t* __restrict__ Rt,
                                                  const uint32_t* __restrict__ scale,
                                                  const uint32_t* __restrict__ tab_g,
                                                  const uint32_t* __restrict__ tab_h, uint8_t* __restrict__ eq) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const uint32_t re = ridx[2 * c], ra = ridx[2 * c + 1];
  const bool tab = re >> 31;
  sc x, f;
  const bool scaled = tab && scale;
  if (scaled) sc_load(f, scale + 8 * (size_t)(accuser[c] - 1));
  ge_p3 acc, r;
  ge_identity(acc);
  sc_load(x, sr + 8 * (2 * c));  // g * share
  if (scaled) sc_mont_mul(x, x, f);
  combw_mul_add(acc, x, tab_g);
  pt_load_aos(r, tab ? Rt : Rh, ra & 0x7fffffffu);
  eq[2 * c + 1] = ristretto_eq(acc, r) ? 1 : 0;
  sc_load(x, sr + 8 * (2 * c + 1));  // + h * randomness
  if (scaled) sc_mont_mul(x, x, f);
  combw_mul_add(acc, x, tab_h);
  pt_load_aos(r, tab ? Rt : Rh, re & 0x7fffffffu);
  eq[2 * c] = ristretto_eq(acc, r) ? 1 : 0;
}

void c3_check(size_t C, const uint32_t* accuser, const uint32_t* sr, const uint32_t* ridx, const uint32_t* Rh,
              const uint32_t* Rt, const uint32_t* scale, const uint32_t* tab_g, const uint32_t* tab_h, uint8_t* eq,
              hipStream_t stream) {
  if (!C) return;
  hipLaunchKernelGGL(k_c3_check, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, stream, C, accuser, sr, ridx, Rh, Rt,
                     scale, tab_g, tab_h, eq);
}

// Verdict of complaint c as Phases<Phase4>::proceed treats it (committee.rs:636-670): 4 the accused is
// disqualified (:639), 5 it has no phase-3 broadcast -- absent, or its A row does not decode -- so the
// complaint holds unverified (:643), else the codes of dkg_complaint3_verify.  rowok [2 arows] decode
// flags of the E rows then the A rows, indexed by the commitment row crow[c] (k_c3_prep); qualified /
// fetched3 (may be null: all 1) are per dealer, indexed by the accused's 1-based dealer row drow[c].
// One ceremony passes `accused` for both and arows = n; a batch passes the gathered row and g n +
// accused.
__global__ __launch_bounds__(256) void k_c3_final(size_t C, size_t arows, const uint32_t* __restrict__ crow,
                                                  const uint32_t* __restrict__ drow,
                                                  const uint8_t* __restrict__ rowok,
                                                  const uint8_t* __restrict__ qualified,
                                                  const uint8_t* __restrict__ fetched3, const uint8_t* __restrict__ eq,
                                                  int32_t* __restrict__ verdict) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const size_t i = crow[c] - 1, d = drow[c] - 1;
  int32_t v;
  if (qualified && !qualified[d]) v = 4;
  else if ((fetched3 && !fetched3[d]) || !rowok[arows + i]) v = 5;
  else if (!rowok[i]) v = -1;
  else if (!eq[2 * c]) v = 3;     // FalseClaimedEquality (broadcast.rs:129-130)
  else if (eq[2 * c + 1]) v = 2;  // FalseClaimedInequality (:131-132)
  else v = 0;
  verdict[c] = v;
}

void c3_final(size_t C, size_t arows, const uint32_t* crow, const uint32_t* drow, const uint8_t* rowok,
              const uint8_t* qualified, const uint8_t* fetched3, const uint8_t* eq, int32_t* verdict,
              hipStream_t stream) {
  if (!C) return;
  hipLaunchKernelGGL(k_c3_final, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, stream, C, arows, crow, drow, rowok,
                     qualified, fetched3, eq, verdict);
}

// ------------------------------------------------------------------ batches of ceremonies: gathers, masks, dissent
// The complaint stage of a batch (runtime.hip batch_complaints) addresses B stacked ceremonies: dealer
// row g n + i is dealer i of ceremony g.  Only the accused rows are decoded a second time: the host
// lists the distinct accused dealer rows (0-based, `rows` [R]) and this kernel copies their compressed
// commitments into out [R][N][8] -- and, with srcA, the same rows of A behind them ([2R][N][8], the E
// rows then the A rows, as k_c3_prep addresses them).  One thread per 16 bytes.
__global__ __launch_bounds__(256) void k_gather_rows(size_t R, size_t N, const uint32_t* __restrict__ rows,
                                                     const uint4* __restrict__ srcE, const uint4* __restrict__ srcA,
                                                     uint4* __restrict__ out) {
  const size_t q = 2 * N;  // uint4 per row
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (srcA ? 2 : 1) * R * q) return;
  const size_t r = idx / q, w = idx % q;
  const bool a = r >= R;
  const size_t src = (size_t)rows[a ? r - R : r] * q + w;
  out[idx] = a ? srcA[src] : srcE[src];
}

void gather_rows(size_t R, size_t N, const uint32_t* rows, const uint32_t* srcE, const uint32_t* srcA, uint32_t* out,
                 hipStream_t stream) {
  const size_t total = (srcA ? 2 : 1) * R * 2 * N;
  if (!total) return;
  hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, R, N, rows,
                     (const uint4*)srcE, (const uint4*)srcA, (uint4*)out);
}

// enc [C][32 words] = e1_rand | ct_rand | e1_share | ct_share: the pair the accused broadcast to the
// accuser (broadcast.rs:57), from the batch's device-resident ciphertexts, items (dealer row, q, w)
// at ((drow - 1) n + q) 2 + w with w = 0 the randomness.  drow [C]: the accused's 1-based dealer row
// g n + accused, accuser [C] the 1-based recipient within the ceremony.  One thread per 16 bytes.
__global__ __launch_bounds__(256) void k_gather_enc(size_t C, size_t n, const uint32_t* __restrict__ drow,
                                                    const uint32_t* __restrict__ accuser,
                                                    const uint4* __restrict__ e1, const uint4* __restrict__ ct,
                                                    uint4* __restrict__ enc) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 8 * C) return;
  const size_t c = idx >> 3, part = (idx >> 1) & 3, h = idx & 1;  // part: e1_rand, ct_rand, e1_share, ct_share
  const size_t item = ((size_t)(drow[c] - 1) * n + (accuser[c] - 1)) * 2 + (part >> 1);
  enc[idx] = ((part & 1) ? ct : e1)[2 * item + h];
}

void gather_enc(size_t C, size_t n, const uint32_t* drow, const uint32_t* accuser, const uint32_t* e1,
                const uint32_t* ct, uint32_t* enc, hipStream_t stream) {
  if (!C) return;
  hipLaunchKernelGGL(k_gather_enc, dim3((unsigned)((8 * C + 255) / 256)), dim3(256), 0, stream, C, n, drow, accuser,
                     (const uint4*)e1, (const uint4*)ct, (uint4*)enc);
}

// The verdicts as the rounds' masks over the V dealer rows.  Round 2 (threads [0, C2); committee.rs:381-394):
// a verdict 0 clears cmask[accused row] and sets pair[accused row][accuser], the proven-pair matrix
// k_dissent reads.  Round 4 (threads [C2, C2 + C4); :643, :664-669): a verdict 0 or 5 sets
// proven4[accused row].  The caller presets cmask to 1 and pair / proven4 to 0.  Several complaints
// may write one byte: they all write the same value (plain byte stores).
__global__ __launch_bounds__(256) void k_proven_masks(size_t C2, size_t n, const uint32_t* __restrict__ drow2,
                                                      const uint32_t* __restrict__ accuser2,
                                                      const int32_t* __restrict__ verdict2, size_t C4,
                                                      const uint32_t* __restrict__ drow4,
                                                      const int32_t* __restrict__ verdict4, uint8_t* __restrict__ cmask,
                                                      uint8_t* __restrict__ pair, uint8_t* __restrict__ proven4) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < C2) {
    if (verdict2[idx] != 0) return;
    const size_t d = drow2[idx] - 1;
    cmask[d] = 0;
    pair[d * n + (accuser2[idx] - 1)] = 1;
  } else if (idx < C2 + C4) {
    const size_t c = idx - C2;
    const int32_t v = verdict4[c];
    if (v == 0 || v == 5) proven4[drow4[c] - 1] = 1;
  }
}

void proven_masks(size_t C2, size_t n, const uint32_t* drow2, const uint32_t* accuser2, const int32_t* verdict2,
                  size_t C4, const uint32_t* drow4, const int32_t* verdict4, uint8_t* cmask, uint8_t* pair,
                  uint8_t* proven4, hipStream_t stream) {
  if (!(C2 + C4)) return;
  hipLaunchKernelGGL(k_proven_masks, dim3((unsigned)((C2 + C4 + 255) / 256)), dim3(256), 0, stream, C2, n, drow2,
                     accuser2, verdict2, C4, drow4, verdict4, cmask, pair, proven4);
}

// dissent[g n + j] = the dealers i of ceremony g that receiver j rejected (dec2 [V][n], REJECT = 0)
// without a proven complaint of its own against them (pair [V][n], k_proven_masks).  Thread = (g, j):
// consecutive lanes read consecutive bytes of each dealer row.
__global__ __launch_bounds__(256) void k_dissent(size_t V, size_t n, const uint8_t* __restrict__ dec2,
                                                 const uint8_t* __restrict__ pair, int32_t* __restrict__ dissent) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= V) return;
  const size_t g = idx / n, j = idx % n;
  int32_t v = 0;
  for (size_t i = 0; i < n; i++) {
    const size_t at = (g * n + i) * n + j;
    v += dec2[at] == 0 && !pair[at];
  }
  dissent[idx] = v;
}

void dissent_rows(size_t V, size_t n, const uint8_t* dec2, const uint8_t* pair, int32_t* dissent, hipStream_t stream) {
  if (!V) return;
  hipLaunchKernelGGL(k_dissent, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, stream, V, n, dec2, pair, dissent);
}

// out[i] = dok[column of dealer i of segment seg], i < D: a segment's per-dealer flags out of the
// verification's interleaved column layout (the inverse of and_dealer_mask's addressing)
__global__ __launch_bounds__(256) void k_segment_mask(size_t D, uint32_t nseg, uint32_t seg,
                                                      const uint8_t* __restrict__ dok, uint8_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D) return;
  out[i] = dok[(i / 64) * 64 * nseg + seg * 64 + i % 64];
}

void segment_mask(size_t D, int nseg, int seg, const uint8_t* dok, uint8_t* out, hipStream_t stream) {
  if (!D) return;
  hipLaunchKernelGGL(k_segment_mask, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, stream, D, (uint32_t)nseg,
                     (uint32_t)seg, dok, out);
}

// ------------------------------------------------------------------ dealer-sharded ceremonies: a rank's own complaints
// A rank verifies the complaints against its D dealers (runtime.hip shard_complaints).  Its fused round-2/4
// pass has already evaluated P^E_i(j) and P^A_i(j) for every receiver j of every one of them, so the
// complaints' evaluation items are elements of that pass's R: dealer group q of 64 holds its E rows in
// columns [128 q, 128 q + 64) and its A rows in [128 q + 64, 128 q + 128) (verify_device, two segments),
// and the recombined value of (column, receiver j) is element column * n + j - 1 (the piece-0 slot).
// ridx [items C] as k_cv_check (items = 1: the E row) and k_c3_check (items = 2: E then A) read it.  lrow
// [C]: the accused's 1-based row among the rank's dealers; accuser [C] 1-based; rowok [2D]: the E rows
// then the A rows decode.  A complaint with a row that does not decode reads no element of R: all its
// items name element 0 of Rh (bit 31 clear), and k_*_final give its verdict from rowok alone.
__global__ __launch_bounds__(256) void k_shard_ridx(size_t C, uint32_t items, size_t D, size_t n,
                                                    const uint32_t* __restrict__ lrow,
                                                    const uint32_t* __restrict__ accuser,
                                                    const uint8_t* __restrict__ rowok, uint32_t* __restrict__ ridx) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const size_t r = lrow[c] - 1, j = accuser[c] - 1;
  bool ok = rowok[r] != 0;
  if (items == 2) ok = ok && rowok[D + r] != 0;
  for (uint32_t s = 0; s < items; s++) {
    const size_t col = (r / 64) * 128 + (size_t)s * 64 + r % 64;
    ridx[items * c + s] = ok ? 0x80000000u | (uint32_t)(col * n + j) : 0u;
  }
}

void shard_ridx(size_t C, int items, size_t D, size_t n, const uint32_t* lrow, const uint32_t* accuser,
                const uint8_t* rowok, uint32_t* ridx, hipStream_t stream) {
  if (!C) return;
  hipLaunchKernelGGL(k_shard_ridx, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, stream, C, (uint32_t)items, D, n,
                     lrow, accuser, rowok, ridx);
}

// The flag words a rank sends beside its packed rows, flags [rows] (rows past D zero): bit 0 some
// verdict-0 round-2 complaint against the dealer (cmask == 0; cmask null: no such round), bit 1 some
// round-4 complaint against it holds (proven4), bit 2 it has no usable phase-3 broadcast (its A row does
// not decode, a_dec == 0, or fetched3 == 0; fetched3 null = all present).
__global__ __launch_bounds__(256) void k_shard_flags(size_t D, size_t rows, const uint8_t* __restrict__ cmask,
                                                     const uint8_t* __restrict__ proven4,
                                                     const uint8_t* __restrict__ a_dec,
                                                     const uint8_t* __restrict__ fetched3,
                                                     uint32_t* __restrict__ flags) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  uint32_t f = 0;
  if (i < D) {
    if (cmask && !cmask[i]) f |= 1u;
    if (proven4[i]) f |= 2u;
    if (!a_dec[i] || (fetched3 && !fetched3[i])) f |= 4u;
  }
  flags[i] = f;
}

void shard_flags(size_t D, size_t rows, const uint8_t* cmask, const uint8_t* proven4, const uint8_t* a_dec,
                 const uint8_t* fetched3, uint32_t* flags, hipStream_t stream) {
  if (!rows) return;
  hipLaunchKernelGGL(k_shard_flags, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, D, rows, cmask, proven4,
                     a_dec, fetched3, flags);
}

// A rank's partial of dissent[j]: its dealers i that receiver j rejected (dec2 [D][n], REJECT = 0) without
// a proven complaint of its own against them (pair [D][n], k_proven_masks).  Thread = receiver:
// consecutive lanes read consecutive bytes of each row.
__global__ __launch_bounds__(256) void k_shard_dissent(size_t D, size_t n, const uint8_t* __restrict__ dec2,
                                                       const uint8_t* __restrict__ pair, int32_t* __restrict__ dissent) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  int32_t v = 0;
  for (size_t i = 0; i < D; i++) v += dec2[i * n + j] == 0 && !pair[i * n + j];
  dissent[j] = v;
}

void shard_dissent(size_t D, size_t n, const uint8_t* dec2, const uint8_t* pair, int32_t* dissent, hipStream_t stream) {
  if (!n) return;
  hipLaunchKernelGGL(k_shard_dissent, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, D, n, dec2, pair,
                     dissent);
}

// The combine's side of the flag words: flags [n] (compacted) -> cmask[i] = bit 0 clear, proven4[i] = bit 1,
// a_ok[i] = bit 2 clear.
__global__ __launch_bounds__(256) void k_flag_masks(size_t n, const uint32_t* __restrict__ flags,
                                                    uint8_t* __restrict__ cmask, uint8_t* __restrict__ proven4,
                                                    uint8_t* __restrict__ a_ok) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t f = flags[i];
  cmask[i] = (f & 1u) ? 0 : 1;
  proven4[i] = (f & 2u) ? 1 : 0;
  a_ok[i] = (f & 4u) ? 0 : 1;
}

void flag_masks(size_t n, const uint32_t* flags, uint8_t* cmask, uint8_t* proven4, uint8_t* a_ok, hipStream_t stream) {
  if (!n) return;
  hipLaunchKernelGGL(k_flag_masks, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, flags, cmask, proven4,
                     a_ok);
}

// out[j] = sum over the ws gathered rank blocks of in[r][j] (the ranks' dissent partials, [ws][n])
__global__ __launch_bounds__(256) void k_sum_partials_i32(size_t ws, size_t n, const int32_t* __restrict__ in,
                                                          int32_t* __restrict__ out) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  int32_t v = 0;
  for (size_t r = 0; r < ws; r++) v += in[r * n + j];
  out[j] = v;
}

void sum_partials_i32(size_t ws, size_t n, const int32_t* in, int32_t* out, hipStream_t stream) {
  if (!n) return;
  hipLaunchKernelGGL(k_sum_partials_i32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ws, n, in, out);
}

}  // namespace dkgk
