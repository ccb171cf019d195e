// The chained builder of the radix-2^BITS combs (points.h CombGeo): the tables k_build_combw
// (kernels.hip) writes -- entry (w, d) = d 2^(BITS w) B in affine Niels form at
// (w ENTRIES + d - 1) COMBW_STRIDE words -- for about one mixed addition and a share of one inversion
// per entry, where k_build_combw's thread pays BITS w doublings, a chain for d and an inversion of its
// own.  Three launches:
//   k_comb_wchain  lanes = bases: one doubling chain per base leaves B_w = 2^(BITS w) B of every window
//                  (raw X, Y, Z) in the scratch -- BITS (WINDOWS - 1) ~ 250 doublings, the builder's
//                  latency floor;
//   k_comb_waff    one lane per (base, window): B_w to affine Niels form in place;
//   k_comb_chain   one lane per chunk of S consecutive entries of a (base, window): the start
//                  (c S + 1) B_w by a per-lane double-and-add, then P_d = P_(d-1) + B_w by ge_madd, the
//                  chunk's Z inverted together (Montgomery's trick).
// ge_madd is the complete unified addition (ge25519.h): a doubling (d = 2), the identity (B = 0, where
// every entry comes out as (1, 1, 0)) and points of small order take the same path, and no Z it
// produces is zero -- so the shared inversion needs no zero handling.
// The closing sequence of an entry is k_build_combw's, operation for operation (comb_entry_put), so
// the entries' limb bounds are the ones the consumers' bound model assumes (tools/fe_bounds.py); the
// words themselves may differ from k_build_combw's (another representative of the same field
// element), the canonical encodings do not (dkg_comb_entries).
#include "comb_build.h"
#include "points.h"

namespace dkgk {

// Entries per thread of k_comb_chain (a power of two, 2 .. 16): the prefix products of a chunk wait
// for the inverse in LDS (40 B per entry and lane), which sets the occupancy (k_comb_chain).  Chosen
// per radix by measurement: DESIGN.md section 4, profiles/comb_build_time.json.
#ifndef DKG_COMBW_CHUNK
#define DKG_COMBW_CHUNK 8
#endif
#ifndef DKG_KEY_COMB_CHUNK
#define DKG_KEY_COMB_CHUNK 16
#endif

template <int BITS>
constexpr int comb_chunk() {
  return BITS == DKG_COMBW_BITS ? DKG_COMBW_CHUNK : DKG_KEY_COMB_CHUNK;
}

// one entry slot (COMBW_STRIDE = 32 words, 128-B aligned) as eight 16-B accesses: three field
// elements and two zero words
DKG_DEV void slot_put(uint32_t* __restrict__ s, const fe& a, const fe& b, const fe& c) {
  uint32_t w[32];
#pragma unroll
  for (int i = 0; i < 10; i++) {
    w[i] = a.v[i];
    w[10 + i] = b.v[i];
    w[20 + i] = c.v[i];
  }
  w[30] = 0;
  w[31] = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) st16<false>(s + 4 * k, w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}
DKG_DEV void slot_get(fe& a, fe& b, fe& c, const uint32_t* s) {
  uint32_t w[32];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const u32x4_t v = *reinterpret_cast<const u32x4_t*>(s + 4 * k);
    w[4 * k] = v.x;
    w[4 * k + 1] = v.y;
    w[4 * k + 2] = v.z;
    w[4 * k + 3] = v.w;
  }
#pragma unroll
  for (int i = 0; i < 10; i++) {
    a.v[i] = w[i];
    b.v[i] = w[10 + i];
    c.v[i] = w[20 + i];
  }
}

// The entry of the point (X : Y : Z) with zi = 1 / Z: k_build_combw's closing sequence.
DKG_DEV void comb_entry_put(uint32_t* __restrict__ out, const fe& X, const fe& Y, const fe& zi) {
  fe x, y, ypx, ymx, t, d2;
  fe_ld(d2, ge_const::D2);
  fe_mul(x, X, zi);
  fe_mul(y, Y, zi);
  fe_add(ypx, y, x);
  fe_carry(ypx, ypx);
  fe_sub(ymx, y, x);
  fe_carry(ymx, ymx);
  fe_mul(t, x, y);
  fe_mul(t, t, d2);
  slot_put(out, ypx, ymx, t);
}

// B_w of base e0 + lane for every window, raw (X, Y, Z), at wb + (base WINDOWS + w) 32 words.
template <int BITS>
__global__ __launch_bounds__(64) void k_comb_wchain(const uint32_t* __restrict__ ext, size_t stride, size_t e0,
                                                    size_t count, uint32_t* __restrict__ wb) {
  using G = CombGeo<BITS>;
  const size_t b = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= count) return;
  ge_p3 p;
  pt_load(p, ext, stride, e0 + b);
  uint32_t* out = wb + b * G::WINDOWS * COMBW_STRIDE;
#pragma unroll 1
  for (int w = 0; w < G::WINDOWS; w++) {
    slot_put(out + (size_t)w * COMBW_STRIDE, p.X, p.Y, p.Z);
    if (w + 1 < G::WINDOWS) {
#pragma unroll 1
      for (int i = 0; i < BITS; i++) ge_dbl<false>(p, p);  // a doubling reads no T
    }
  }
}

// the scratch's raw B_w to affine Niels form, in place
__global__ __launch_bounds__(64) void k_comb_waff(size_t total, uint32_t* __restrict__ wb) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= total) return;
  uint32_t* s = wb + i * COMBW_STRIDE;
  fe X, Y, Z, zi;
  slot_get(X, Y, Z, s);
  fe_invert(zi, Z);
  comb_entry_put(s, X, Y, zi);
}

// Lane (w, c) = blockIdx.x * 64 + lane of base blockIdx.y: entries c S + 1 .. c S + S of window w.
// The chunk's prefix products Z_0 .. Z_k wait for the inverse in LDS, lane-interleaved (word i of
// product k of lane l at (k 10 + i) 64 + l: conflict-free) -- S x 2.5 KiB per wave, so S = 8 leaves two
// waves per SIMD and S = 16 one.  Held in registers instead (80 VGPRs at S = 8, the chunk loops
// unrolled) the kernel met the 256-VGPR cap of two waves and spilled 540 B per lane.  The kernel takes
// 180 VGPRs: a smaller chunk's LDS would admit four waves, but under their 128-VGPR cap it spills
// (200 B per lane at S = 4), so two waves it is for every S <= 8.
template <int S>
constexpr int comb_chain_waves() { return S <= 8 ? 2 : 1; }
template <int BITS, int S>
__global__ __launch_bounds__(64, comb_chain_waves<S>()) void k_comb_chain(const uint32_t* __restrict__ wb,
                                                                          uint32_t* __restrict__ tab) {
  using G = CombGeo<BITS>;
  constexpr unsigned CHUNKS = G::ENTRIES / S;
  static_assert(S >= 2 && S <= 16 && (S & (S - 1)) == 0 && G::ENTRIES % S == 0, "chunk: a power of two, 2 .. 16");
  static_assert(CHUNKS % 64 == 0 || 64 % CHUNKS == 0, "a wave's lanes share their top multiplier");
  __shared__ uint32_t lds[S * 10 * 64];
  const unsigned gid = blockIdx.x * 64 + threadIdx.x;
  if (gid >= G::WINDOWS * CHUNKS) return;
  const unsigned w = gid / CHUNKS, c = gid % CHUNKS;
  uint32_t* pre = lds + threadIdx.x;
  ge_aff bw;
  slot_get(bw.ypx, bw.ymx, bw.xy2d, wb + ((size_t)blockIdx.y * G::WINDOWS + w) * COMBW_STRIDE);
  // the start (c S + 1) B_w: double-and-add from the identity over the bits of the lane's multiplier,
  // from the top bit of the wave's largest (its lanes are consecutive chunks: the high bits agree, and
  // a bit no lane has costs a doubling without T)
  const uint32_t m = c * S + 1;
  const uint32_t mtop = __builtin_amdgcn_readfirstlane(((gid | 63u) % CHUNKS) * S + 1);
  ge_p3 p;
  ge_identity(p);
#pragma unroll 1
  for (int i = 31 - __builtin_clz(mtop); i >= 0; i--) {
    const bool bit = (m >> i) & 1u;
    const bool any = __builtin_amdgcn_ballot_w64(bit) != 0;
    ge_dbl_rt(p, p, any || i == 0);
    if (bit) ge_madd(p, p, bw);
  }
  uint32_t* slot = tab + (size_t)blockIdx.y * G::WORDS + ((size_t)w * G::ENTRIES + (size_t)c * S) * COMBW_STRIDE;
  // forward: entry k's raw (X, Y, Z) waits in its own slot, the running product of the Z in pre[k]
  fe run;
  fe_copy(run, p.Z);
#pragma unroll 1
  for (int k = 0; k < S; k++) {
    slot_put(slot + k * COMBW_STRIDE, p.X, p.Y, p.Z);
#pragma unroll
    for (int i = 0; i < 10; i++) pre[(k * 10 + i) * 64] = run.v[i];
    if (k + 1 < S) {
      ge_madd(p, p, bw);
      fe_mul(run, run, p.Z);
    }
  }
  // backward: run = 1 / (Z_0 .. Z_k); 1 / Z_k = run * (Z_0 .. Z_(k-1)), then run *= Z_k.  No Z is zero
  // (complete formulas), so the product is invertible.
  fe_invert(run, run);
#pragma unroll 1
  for (int k = S - 1; k > 0; k--) {
    uint32_t* s = slot + k * COMBW_STRIDE;
    fe X, Y, Z, zi, pk;
    slot_get(X, Y, Z, s);
#pragma unroll
    for (int i = 0; i < 10; i++) pk.v[i] = pre[((k - 1) * 10 + i) * 64];
    fe_mul(zi, run, pk);
    fe_mul(run, run, Z);
    comb_entry_put(s, X, Y, zi);
  }
  {
    fe X, Y, Z;
    slot_get(X, Y, Z, slot);
    comb_entry_put(slot, X, Y, run);
  }
}

__global__ __launch_bounds__(64) void k_comb_entries_bytes(const uint32_t* __restrict__ ent, uint32_t count,
                                                           uint32_t* __restrict__ out) {
  const uint32_t e = blockIdx.x * 64 + threadIdx.x;
  if (e >= count) return;
  fe a, b, c;
  slot_get(a, b, c, ent + (size_t)e * COMBW_STRIDE);
  uint32_t s[8];
  uint32_t* o = out + (size_t)e * 24;
  fe_tobytes32(s, a);
  st_words8(o, s);
  fe_tobytes32(s, b);
  st_words8(o + 8, s);
  fe_tobytes32(s, c);
  st_words8(o + 16, s);
}

template <int BITS>
void build_comb_chained_r(const uint32_t* ext, size_t stride, size_t e0, uint32_t* tab, uint32_t* scratch,
                          hipStream_t stream, size_t count) {
  using G = CombGeo<BITS>;
  constexpr int S = comb_chunk<BITS>();
  const size_t total = count * G::WINDOWS;
  hipLaunchKernelGGL(k_comb_wchain<BITS>, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, stream, ext, stride, e0,
                     count, scratch);
  hipLaunchKernelGGL(k_comb_waff, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, stream, total, scratch);
  constexpr unsigned lanes = G::WINDOWS * (G::ENTRIES / S);
  hipLaunchKernelGGL((k_comb_chain<BITS, S>), dim3((lanes + 63) / 64, (unsigned)count), dim3(64), 0, stream, scratch,
                     tab);
}

bool comb_geometry(int kind, int* bits, int* windows, uint32_t* entries, uint32_t* chunk) {
  if (kind != 0 && kind != 1) return false;
  const int b = kind == 0 ? DKG_COMBW_BITS : DKG_KEY_COMB_BITS;
  if (bits) *bits = b;
  if (windows) *windows = 256 / b + 1;
  if (entries) *entries = 1u << (b - 1);
  if (chunk) *chunk = kind == 0 ? comb_chunk<DKG_COMBW_BITS>() : comb_chunk<DKG_KEY_COMB_BITS>();
  return true;
}

size_t comb_chain_scratch_words(int kind, size_t count) {
  int windows = 0;
  if (!comb_geometry(kind, nullptr, &windows, nullptr, nullptr)) return 0;
  return count * (size_t)windows * COMBW_STRIDE;
}

void build_comb_chained(int kind, const uint32_t* ext, size_t stride, size_t e0, uint32_t* tab, uint32_t* scratch,
                        hipStream_t stream, size_t count) {
  if (!count) return;
  if (kind == 0) build_comb_chained_r<DKG_COMBW_BITS>(ext, stride, e0, tab, scratch, stream, count);
  else build_comb_chained_r<DKG_KEY_COMB_BITS>(ext, stride, e0, tab, scratch, stream, count);
}

void comb_entries_bytes(int kind, const uint32_t* tab, int window, uint32_t first, uint32_t count, uint32_t* out,
                        hipStream_t stream) {
  uint32_t entries = 0;
  if (!count || !comb_geometry(kind, nullptr, nullptr, &entries, nullptr)) return;
  const uint32_t* ent = tab + ((size_t)window * entries + first) * COMBW_STRIDE;
  hipLaunchKernelGGL(k_comb_entries_bytes, dim3((count + 63) / 64), dim3(64), 0, stream, ent, count, out);
}

}  // namespace dkgk
