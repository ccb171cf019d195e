// Full (encrypted-share) mode for batches of independent ceremonies: the two per-item scalar
// multiplications of hybrid.hip with per-ceremony keys.  Ceremony c's dealers are rows c*n .. c*n+n-1;
// item (c, i, q, w) = dealer i of ceremony c to recipient q, w = 0 the randomness s', w = 1 the share
// s, at index ((c*n + i)*n + q)*2 + w; recipient q of ceremony c owns key c*n + q.
//   encrypt: K = pk_{c,q} * r.  A key serves only the 2n items of its own ceremony, so the single
//            ceremony's radix-2^10 comb (1.7 MB per key) costs more to build than it saves.  Each key
//            gets a signed radix-16 comb instead -- 64 windows x 8 multiples in cached form, 80 KiB --
//            built with lanes = keys (k_benc_tab) into a table that lives for one chunk of
//            ceremonies; the items then take 64 complete additions and no doubling (k_benc_mul).  The
//            2n items of a key sit in the same waves and walk the windows in step, so a window's eight
//            entries (1.3 KB) are read from the vector cache.  Only pk enters: the dealer side never
//            sees a secret key.  e1 = g * r is the generator's shared comb (fixed_base).
//   decrypt: K = sk_{c,q} * e1, the width-4 window chain of k_dec_mul_w4 (hybrid.hip) with batched
//            addressing on a flat grid: one wave per (c, q, w, group of 64 dealers).
// decode / encode, sym_xor and dealer_ok are item-indexed already and serve a chunk as D = Bc*n rows.
// The radix-16 combs also serve ONE ceremony's dealer shard (runtime.hip encrypt_device, kind 2): one key
// set of n keys, D != n dealers per key (k_benc_mul's `rows`), where 2 D items per key do not repay a
// radix-2^10 table either.
#include "kernels.h"
#include "points.h"
#include "hybrid_dev.h"

namespace dkgk {

constexpr int BENC_WINDOWS = 64, BENC_DIGITS = 8;
constexpr size_t BENC_TAB_WORDS = (size_t)BENC_WINDOWS * BENC_DIGITS * PT_WORDS;  // 20,480 words = 80 KiB per key

// The build runs one lane per (key, group of windows): group g first doubles the key 4 * 64/G * g
// times, then walks its 64/G windows.  Lanes = keys alone (G = 1) leave a chunk of 16,384 keys at one
// wave per CU for ~550 dependent additions; G groups shorten that chain at the price of the leading
// doublings.  blockIdx.y = g, so a wave's lanes share their trip counts.
#ifndef DKG_BENC_TAB_GROUPS
#define DKG_BENC_TAB_GROUPS 8
#endif
static_assert(BENC_WINDOWS % DKG_BENC_TAB_GROUPS == 0, "window groups must divide the 64 windows");

DKG_DEV void benc_put(uint32_t* __restrict__ e, const ge_cached& c) {
  const uint32_t* w = reinterpret_cast<const uint32_t*>(&c);
#pragma unroll
  for (int k = 0; k < PT_WORDS / 4; k++) st16<false>(e + 4 * k, w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}

// tab[key][w][d-1] = d * 16^w * P_key (d = 1..8) in cached form (Y+X, Y-X, 2Z, 2dT), 40 words per entry.
__global__ __launch_bounds__(64, 2) void k_benc_tab(size_t keys, const uint32_t* __restrict__ pk_ext, size_t stride,
                                                    uint32_t* __restrict__ tab) {
  constexpr int WPG = BENC_WINDOWS / DKG_BENC_TAB_GROUPS;
  const size_t key = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (key >= keys) return;
  const int g = blockIdx.y;
  ge_p3 m;
  pt_load(m, pk_ext, stride, key);
  const int lead = 4 * WPG * g;
#pragma unroll 1
  for (int b = 0; b < lead; b++) ge_dbl_lean(m, m, b == lead - 1);  // T only for the additions that follow
  uint32_t* out = tab + key * BENC_TAB_WORDS + (size_t)g * WPG * BENC_DIGITS * PT_WORDS;
#pragma unroll 1
  for (int w = 0; w < WPG; w++) {
    ge_cached c;
    ge_to_cached(c, m);  // 1 * B_w
    benc_put(out, c);
#pragma unroll 1
    for (int d = 1; d < BENC_DIGITS; d++) {
      ge_add(m, m, c);   // (d + 1) * B_w
      ge_cached cd;
      ge_to_cached(cd, m);
      benc_put(out + d * PT_WORDS, cd);
    }
    ge_dbl_lean(m, m, true);  // B_{w+1} = 16 B_w = 2 * (8 B_w)
    out += BENC_DIGITS * PT_WORDS;
  }
}

void benc_tab(size_t keys, const uint32_t* pk_ext, size_t stride, uint32_t* tab, hipStream_t stream) {
  if (!keys) return;
  hipLaunchKernelGGL(k_benc_tab, dim3((unsigned)((keys + 63) / 64), (unsigned)DKG_BENC_TAB_GROUPS), dim3(64), 0, stream,
                     keys, pk_ext, stride, tab);
}

size_t benc_tab_words() { return BENC_TAB_WORDS; }

// K = pk_key * r for the items of `keys` keys (key sets of n recipients stacked key-wise, `rows` dealers
// per key set: rows = n for a batch's ceremonies, rows = D for one ceremony's dealer shard).  Every wave
// serves one key: S = ceil(2 rows / 64) waves per key, lane j of them the item (dealer j / 2, w = j % 2);
// key c*n + q serves items ((c*rows + i)*n + q)*2 + w, i < rows.  Only the index computation reads rows.
// r [items][8] canonical scalars (< 2^253: the top radix-16 digit then absorbs the recoding's carry);
// K_ext SoA [40][count].
#ifndef DKG_BENC_WAVES
#define DKG_BENC_WAVES 2
#endif
#ifndef DKG_BENC_IL
#define DKG_BENC_IL 1
#endif
__global__ __launch_bounds__(256, DKG_BENC_WAVES) void k_benc_mul(size_t keys, size_t n, const uint32_t* __restrict__ r,
                                                                  const uint32_t* __restrict__ tab,
                                                                  uint32_t* __restrict__ K_ext, size_t count,
                                                                  size_t rows) {
  const size_t S = (2 * rows + 63) / 64;
  const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const size_t key = wave / S;
  if (key >= keys) return;
  const size_t j = (wave % S) * 64 + (threadIdx.x & 63);
  if (j >= 2 * rows) return;
  const size_t c = key / n, q = key % n, i = j >> 1, w = j & 1;
  const size_t idx = ((c * rows + i) * n + q) * 2 + w;
  const uint32_t* kt = tab + key * BENC_TAB_WORDS;
  sc x;
  sc_load(x, r + 8 * idx);
  ge_p3 acc;
  ge_identity(acc);
  int carry = 0;
#pragma unroll 1
  for (int win = 0; win < BENC_WINDOWS; win++) {
    const int wi = win >> 3;  // wave-uniform word select
    uint32_t word = x.v[0];
#pragma unroll
    for (int k = 1; k < 8; k++) word = (wi == k) ? x.v[k] : word;
    int d = (int)((word >> (4 * (win & 7))) & 15u) + carry;  // recentred as dalek's to_radix_16
    carry = (d + 8) >> 4;
    d -= carry << 4;
    const int ad = d < 0 ? -d : d;
    const bool neg = d < 0, zero = ad == 0;
    const uint4* p = reinterpret_cast<const uint4*>(kt + (size_t)(win * BENC_DIGITS + (zero ? 0 : ad - 1)) * PT_WORDS);
    uint4 e[PT_WORDS / 4];
#pragma unroll
    for (int k = 0; k < PT_WORDS / 4; k++) e[k] = p[k];
    const uint32_t* ew = reinterpret_cast<const uint32_t*>(e);
    ge_cached qc;
#pragma unroll
    for (int k = 0; k < 10; k++) {  // digit 0 adds the identity (1, 1, 2, 0): one code path for every lane
      qc.YpX.v[k] = zero ? (k == 0 ? 1u : 0u) : ew[k];
      qc.YmX.v[k] = zero ? (k == 0 ? 1u : 0u) : ew[10 + k];
      qc.Z2.v[k] = zero ? (k == 0 ? 2u : 0u) : ew[20 + k];
      qc.T2d.v[k] = zero ? 0u : ew[30 + k];
    }
    ge_add_signed<DKG_BENC_IL != 0>(acc, acc, qc, neg);
  }
  pt_store(K_ext, count, idx, acc);
}

void benc_mul(size_t keys, size_t n, size_t rows, const uint32_t* r, const uint32_t* tab, uint32_t* K_ext,
              size_t count, hipStream_t stream) {
  if (!keys || !n || !rows) return;
  const size_t waves = keys * ((2 * rows + 63) / 64);
  hipLaunchKernelGGL(k_benc_mul, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, keys, n, r, tab, K_ext,
                     count, rows);
}

// Width-4 signed window recoding of a canonical scalar (wNAF: digits 0, +-1, +-3, +-5, +-7), as
// k_dec_mul_w4 computes it: dig the digits by bit, nzb / nzd the nonzero ones top first.
DKG_DEV int w4_recode(const uint32_t* __restrict__ sk8, int8_t* dig, int16_t* nzb, int8_t* nzd) {
  uint32_t k[9];
  for (int j = 0; j < 8; j++) k[j] = sk8[j];
  k[8] = 0;
  for (int b = 0; b < 288; b++) {
    int8_t d = 0;
    if (k[0] & 1u) {
      int v = (int)(k[0] & 15u);
      if (v >= 8) v -= 16;
      d = (int8_t)v;
      if (v > 0) {  // k -= v
        uint32_t sub = (uint32_t)v;
        for (int wi = 0; wi < 9; wi++) {
          const uint32_t old = k[wi];
          k[wi] = old - sub;
          if (old >= sub) break;
          sub = 1u;
        }
      } else {      // k += -v
        uint32_t add = (uint32_t)(-v);
        for (int wi = 0; wi < 9; wi++) {
          const uint32_t old = k[wi];
          k[wi] = old + add;
          if (k[wi] >= old) break;
          add = 1u;
        }
      }
    }
    dig[b] = d;
    for (int wi = 0; wi < 8; wi++) k[wi] = (k[wi] >> 1) | (k[wi + 1] << 31);
    k[8] >>= 1;
  }
  int c = 0;
  for (int b = 287; b >= 0; b--)
    if (dig[b]) {
      nzb[c] = (int16_t)b;
      nzd[c] = dig[b];
      c++;
    }
  return c;
}

// K = sk_{c,q} * R for the items of a chunk.  Flat grid: workgroup (= wave) wv0 + blockIdx.x is
// (key = c*n + q, w, lane group lg) with lg fastest, its lanes the dealers lg*64 .. of ceremony c; the
// scalar is wave-uniform.  The chain is k_dec_mul_w4's (hybrid.hip): each lane's odd multiples R, 3R,
// 5R, 7R in the global table T (one 40-KB slot per wave of the launch, blockIdx.x), the next addend
// copied into the wave's LDS slot by LDS-DMA during the doublings before it.  SEATS: the item index has
// no recipient axis (k_seat_dec_mul_w4 below); nothing else differs.
template <bool SEATS>
DKG_DEV void bdec_w4_wave(size_t n, size_t LG, size_t wv0, const uint32_t* __restrict__ sk,
                          const uint32_t* __restrict__ R_ext, uint32_t* __restrict__ K_ext, size_t count,
                          uint32_t* __restrict__ T) {
  __shared__ uint32_t qs[PT_WORDS * 64];
  __shared__ int16_t nzb[96];  // bits of the nonzero digits, top first
  __shared__ int8_t nzd[96];   // their digits
  __shared__ int8_t dig[288];  // the recoding (LDS: a private array would live in scratch)
  __shared__ int nnz_s;
  uint32_t* qcol = qs + threadIdx.x;
  const size_t wv = wv0 + blockIdx.x;
  const size_t lg = wv % LG, w = (wv / LG) & 1, key = wv / (2 * LG);
  const size_t c = key / n, q = key % n;
  const size_t i = lg * 64 + threadIdx.x;
  const bool live = i < n;
  const size_t idx = SEATS ? (key * n + (live ? i : 0)) * 2 + w : ((c * n + (live ? i : 0)) * n + q) * 2 + w;
  uint32_t* tb = T + (size_t)blockIdx.x * (4 * PT_WORDS * 64);
  if (threadIdx.x == 0) nnz_s = w4_recode(sk + 8 * key, dig, nzb, nzd);
  // the lane's table of odd multiples
  ge_p3 x;
  if (live) pt_load(x, R_ext, count, idx);
  else ge_identity(x);
  {
    ge_cached cc;
    ge_to_cached(cc, x);
    lds_put_cached(tb + threadIdx.x, cc);  // T[0] = R (global, lane-interleaved like the LDS slot)
    ge_p3 x2;
    ge_dbl<true>(x2, x);
    ge_to_cached(cc, x2);
    lds_put_cached(qcol, cc);              // 2R in the LDS slot
#pragma unroll 1
    for (int m = 1; m < 4; m++) {
      ge_add_lds(x, x, qcol, false);       // (2m+1) R
      ge_to_cached(cc, x);
      lds_put_cached(tb + m * PT_WORDS * 64 + threadIdx.x, cc);
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // table stored, slot reads done
  __syncthreads();
  const int nnz = __builtin_amdgcn_readfirstlane(nnz_s);
  auto fetch = [&](int e) {  // addend of nonzero digit e into the LDS slot (LDS-DMA, one word per instr)
    const int a = (nzd[e] < 0 ? -nzd[e] : nzd[e]) >> 1;
    const uint32_t* src = tb + a * PT_WORDS * 64 + threadIdx.x;
    glds_words<16>((const dec_g_u32*)src, qs);
    glds_words<16>((const dec_g_u32*)(src + 16 * 64), qs + 16 * 64);
    glds_words<8>((const dec_g_u32*)(src + 32 * 64), qs + 32 * 64);
  };
  ge_identity(x);
  if (nnz > 0) {
    fetch(0);
    int b = __builtin_amdgcn_readfirstlane((int)nzb[0]);
#pragma unroll 1
    for (int e = 0; e < nnz; e++) {
      const int be = __builtin_amdgcn_readfirstlane((int)nzb[e]);
      const int de = __builtin_amdgcn_readfirstlane((int)nzd[e]);
#pragma unroll 1
      for (; b > be; b--) ge_dbl_lean<DKG_DEC_IL != 0>(x, x, b - 1 == be);  // T only before the addition
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the DMA'd addend has landed
      __builtin_amdgcn_s_barrier();
      ge_add_lds<DKG_DEC_IL != 0>(x, x, qcol, de < 0, 64, be == 0);  // a doubling follows unless be = 0
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the slot's reads are done
      if (e + 1 < nnz) fetch(e + 1);
    }
#pragma unroll 1
    for (; b > 0; b--) ge_dbl_lean<DKG_DEC_IL != 0>(x, x, b == 1);  // trailing zero digits
  }
  if (live) pt_store(K_ext, count, idx, x);
}

__global__ __launch_bounds__(64, DKG_DEC_W4_WAVES) void k_bdec_mul_w4(size_t n, size_t LG, size_t wv0,
                                                                      const uint32_t* __restrict__ sk,
                                                                      const uint32_t* __restrict__ R_ext,
                                                                      uint32_t* __restrict__ K_ext, size_t count,
                                                                      uint32_t* __restrict__ T) {
  bdec_w4_wave<false>(n, LG, wv0, sk, R_ext, K_ext, count, T);
}

// The same chain for the seats of one operator: key p = seat p's secret key, its items the n pairs
// addressed to it, item (p * n + i) * 2 + w (no recipient axis: the rows-per-key split of k_benc_mul).
__global__ __launch_bounds__(64, DKG_DEC_W4_WAVES) void k_seat_dec_mul_w4(size_t n, size_t LG, size_t wv0,
                                                                          const uint32_t* __restrict__ sk,
                                                                          const uint32_t* __restrict__ R_ext,
                                                                          uint32_t* __restrict__ K_ext, size_t count,
                                                                          uint32_t* __restrict__ T) {
  bdec_w4_wave<true>(n, LG, wv0, sk, R_ext, K_ext, count, T);
}

// waves of one bdec_mul call, and the words of its odd-multiples table (slices of <= DEC_TAB_WAVES)
static size_t bdec_waves(size_t keys, size_t n) { return keys * 2 * ((n + 63) / 64); }

size_t bdec_launch_waves() { return DEC_TAB_WAVES; }

size_t bdec_mul_table_words(size_t keys, size_t n) {
  return std::min(bdec_waves(keys, n), DEC_TAB_WAVES) * 4 * PT_WORDS * 64;
}

void bdec_mul(size_t keys, size_t n, const uint32_t* sk, const uint32_t* R_ext, uint32_t* K_ext, size_t count,
              uint32_t* table, hipStream_t stream) {
  if (!keys || !n) return;
  const size_t waves = bdec_waves(keys, n);
  for (size_t wv0 = 0; wv0 < waves; wv0 += DEC_TAB_WAVES)
    hipLaunchKernelGGL(k_bdec_mul_w4, dim3((unsigned)std::min(DEC_TAB_WAVES, waves - wv0)), dim3(64), 0, stream, n,
                       (n + 63) / 64, wv0, sk, R_ext, K_ext, count, table);
}

void seat_dec_mul(size_t seats, size_t n, const uint32_t* sk, const uint32_t* R_ext, uint32_t* K_ext, size_t count,
                  uint32_t* table, hipStream_t stream) {
  if (!seats || !n) return;
  const size_t waves = bdec_waves(seats, n);
  for (size_t wv0 = 0; wv0 < waves; wv0 += DEC_TAB_WAVES)
    hipLaunchKernelGGL(k_seat_dec_mul_w4, dim3((unsigned)std::min(DEC_TAB_WAVES, waves - wv0)), dim3(64), 0, stream, n,
                       (n + 63) / 64, wv0, sk, R_ext, K_ext, count, table);
}

}  // namespace dkgk
