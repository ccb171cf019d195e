// Host runtime of the MI355X DKG backend: device context, buffer arena, the C ABI of
// include/dkg_amd.h, and the ceremony driver that plays the reference's rounds 1-5
// (committee.rs:124-805) for all parties in one process on one GPU.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <array>
#include <iterator>
#include <map>
#include <memory>
#include <optional>
#include <string>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/dkg_amd.h"
#include "host_crypto.h"
#include "kernels.h"
#include "kernels_ilp.h"
#include "comb_build.h"
#include "seat_finalise.h"
#include "seat_deal.h"

struct dkg_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  std::map<std::string, std::pair<void*, size_t>> bufs;
  std::map<std::string, std::pair<void*, size_t>> hbufs;  // pinned host staging (hbuf), grow-only
  uint32_t* tab_g = nullptr;  // comb table of the generator (15360 words)
  uint32_t* tab_h = nullptr;  // comb table of the commitment key h
  uint32_t* tab_gw = nullptr;  // radix-2^11 combs (global, L2 / MALL-resident) of g and h: commit, check,
  uint32_t* tab_hw = nullptr;  // fixed-base products
  uint8_t h[32] = {0};
  bool have_h = false;
  size_t threshold = 0, nr_members = 0;
  hipEvent_t ev[8] = {};
  // The phase recorder behind dkg_ctx_phase_ms: every family's device-time marks of the current call in record
  // order, mark k on phase_pool[k] (grow-only).  phase_mark adds one, phase_collect turns a tag's marks into
  // "<tag>.<name>" entries after the sync; guarded() clears the list, so a call's uncollected marks end with it.
  struct PhaseMark {
    const char* tag;                    // the family (a literal); null once collected
    int phase;                          // the phase whose segment the mark closes; < 0: a start mark
  };
  std::vector<hipEvent_t> phase_pool;
  std::vector<PhaseMark> phase_marks;
  int receiver_chunk = 0;               // chunk length of the one-party evaluation (0: dkg_receiver_plan_for's rule)
  int last_receiver_chunk = 0;          // the chunk the last such call ran (the largest over its indices)
  size_t ps_slab = 0;                   // rows decoded at a time by dkg_commitment_sum / dkg_public_shares (0: automatic)
  std::map<std::array<size_t, 4>, dkg_receiver_plan> recv_plans;  // dkg_receiver_plan_for by (n, t, x, chunk)
  std::map<std::array<size_t, 3>, std::vector<uint32_t>> pair_digits;  // k_pair_eval's fold_records by (t, x, L)
  static constexpr int MAX_SUB = 8;
  int nsub = 2;                         // dealer-chunk streams of verify_device
  hipStream_t sub[MAX_SUB] = {};
  hipEvent_t fork = nullptr, join[MAX_SUB] = {};
  // round-1 share evaluation on a low-priority side stream beside the first binomial steps
  // (round1_device with overlap_shares): the checks and round 3 wait for shares_done
  hipStream_t side = nullptr;
  hipEvent_t side_fork = nullptr, shares_done = nullptr, pub_done = nullptr;
  hipEvent_t terms_done = nullptr;      // a shard's master-key terms, encoded on the side stream
  bool shares_pending = false;
  bool overlap = true;                  // rounds 2 and 4 as one fused pipeline (verify_rounds)
  int split = 0;                        // degree split U of the difference tables (0: cost model)
  std::vector<uint8_t> key_tabs_pk;     // member keys whose decoded points and combs sit in hy.* (encrypt)
  std::vector<uint8_t> key_tabs16_pk;   // ... and whose radix-16 combs sit in hy16.* (a cache of its own)
  int key_comb = 0;                     // K = pk_q r: 0 radix 2^DKG_KEY_COMB_BITS, except that the sharded
                                        // full calls choose by dkg_key_comb_choice; 1 / 2 force a kind
  int last_key_comb = 0;                // the kind the last encrypt_device used (0: none yet)
  int seat_deal = 0;                    // K = pk r of dkg_party_round1_seats: 0 automatic (DKG_SEAT_DEAL_AUTO), 1
                                        // radix-16 combs per key slot, 2 the joint chain (seat_deal.hip)
  int last_seat_deal = 0;               // the route the last such call ran (0: none yet)
  int seat_eval = 0, seat_eval_chunk = 0;  // the seats' evaluation: 0 dkg_seat_eval_shape's rule, 1 k_seat_horner,
                                           // 2 chunked with this chunk (0: the rule's)
  int last_seat_eval = 0, last_seat_eval_chunk = 0;  // the route and L the last seats call ran (0: none yet)
  uint8_t fb_base[32] = {0};            // dkg_fixed_base_batch: the caller base whose comb sits in fb_tabw
  bool fb_valid = false;
  int comb_build = 0;                   // radix-2^BITS comb builder: 0 automatic (comb_build_auto), 1 one
                                        // thread per entry (k_build_combw), 2 chained (comb_build.hip)
  int last_comb_build = 0;              // the builder the last build ran (0: none yet)
  hipEvent_t cb_ev[2] = {};             // around that build's launches
  int binom_mode = 0;                   // binomial: 0 per-wave Horner loops (k_binom_wave) for
                                        // tables of many column groups, else one launch per step
                                        // with lane pairs (k_binom_pair) for the steps under one
                                        // wave per SIMD; 1 per step, no lane pairs; 2 per step, lane
                                        // pairs for every step; 3 per step as 0; 4 per wave always;
                                        // 5 per wave always, operands prefetched one item ahead
  int step_mode = 0;                    // stepping slots: 0 cost model, 1 whole columns, 2 per piece,
                                        // 3 as 0 without the dead-position repack
  int check_mode = 0;                   // fused round-2/4 checks: 0 one launch, 1 the g and h combs
                                        // in two launches (g*s parked between them)
  int fe_mode = 0;                      // field multiplication per launch: 0 by occupancy, 1 product
                                        // scanning (dkgk), 2 column sums (dkgk_ilp)
  int verify_mode = 0;                  // 0: difference tables (every P_i(j) in the group); 1: interpolation
  size_t vinv_N = 0;                    // key of the cached inverse Vandermonde (v.vinv)
  size_t fallback_rows = 0;             // interpolation mode: rows re-verified the general way
  int last_split = 1;                   // U used by the last verify_device
  size_t last_split_len = 0;            // and its piece length L
  size_t ydig_n = 0, ydig_L = 0;        // key of the cached combine multipliers (v.ydig)
  int combine_mode = 0;                 // recombination: 0 short vectors for U <= 5 (4 with
                                        // projective addends), pairwise JSF chains at U = 2, 4 with
                                        // affine addends; 1 powers of y; 2 = 0; 3 short vectors
                                        // with per-scalar NAF chains at every U
  int last_combine = 0;                 // 1: the last verify_device recombined with powers, 2: short vectors
  int last_binomial = 0;                // 1: the last verify_device ran the per-wave binomial
  int step_formula = 0;                 // stepping additions: 0 dedicated + complete redo of marked
                                        // workgroups, 1 complete formula only
  uint32_t* last_step_flags = nullptr;  // the last verify_device's stepping flags (dedicated mode)
  size_t last_step_flag_words = 0;
  uint32_t* last_bflags = nullptr;      // the last verify_device's per-wave binomial redo flags (v.bflags)
  size_t last_bflag_words = 0;
  // the per-step binomial's dedicated additions: only inside the drivers that check its group flags
  // after their sync and rerun the verification with the complete formula when one is set
  // (receivers_rounds, shard_rows: binom_step_ded = true around the call)
  bool binom_step_ded = false;
  uint32_t* binom_any = nullptr;        // device word: a dedicated per-step binomial marked a group
                                        // since the last verify_rounds began (null: none ran)
  const uint32_t* binom_any_host = nullptr;  // its pinned copy, queued before the caller's sync
  int last_binom_rerun = 0;             // the last guarded driver reran its verification (1) or not
  int addend_mode = 0;                  // short vectors' addends: 0 affine Niels (affine_pieces, mixed
                                        // additions), 1 cached projective (read from R)
  size_t sdig_n = 0, sdig_L = 0, sdig_K = 0;  // key of the cached short multipliers (v.sdig)
  int sdig_jsf = -1;                    // ... and their recoding (0 NAFs, 1 pairwise JSF)
  // the last verify_device's evaluations R[c][j] (point-major, column c = dealer for one segment),
  // their scale b_j 2^256 mod l (null: R holds P(j) itself) and the columns' decode mask: read by the
  // complaint verification, which runs the pipeline without its checks (VerifySeg::dec == null)
  const uint32_t* last_R = nullptr;
  const uint32_t* last_scale = nullptr;
  const uint8_t* last_dok = nullptr;
  int last_dok_nseg = 1;                // its segments (columns interleaved as and_dealer_mask addresses them)
  const uint8_t* last_pok = nullptr;    // its per-point decode flags [last_npad][N], before any dealer mask
  size_t last_npad = 0;
  int complaint_eval = 0;               // P_i(j) of the complaints: 0 by the dealer's complaint count,
                                        // 1 per-pair Horner, 2 difference tables
  int last_complaint_eval = 0;          // dkg_ctx_last_complaint_eval: the sharded proven calls' source
  // round-1 commitments of the ceremony being verified, in extended form on this device (set by
  // the drivers that generate them, ExtScope): verify_device places them instead of decoding the
  // encodings, finalise reads A_i0 from them.  E/A [D][t+1] points, word stride ext_stride.
  const uint32_t* ext_E = nullptr;
  const uint32_t* ext_A = nullptr;
  // round-1 commitments deferred into the verification's chunks (batches, BatchRound1): coefficients
  // [r1_D][N][8]; each chunk's stream computes its dealers' E/A into ext_E / ext_A before its
  // binomial, so one chunk's commitments run beside the other chunk's pipeline
  const uint32_t* r1_a = nullptr;
  const uint32_t* r1_b = nullptr;
  size_t r1_D = 0;
  uint32_t* r1_A0 = nullptr;            // [40][r1_D]: A_i0 of the deferred commitments (finalise)
  size_t ext_stride = 0;
  // share rows [shard_D][shard_n][8] of the last sharded call's dealers [shard_d0, +shard_D)
  // (arena-owned; dkg_ceremony_shard_recon_device reads them after the exchange)
  const uint32_t* shard_s = nullptr;
  size_t shard_n = 0, shard_d0 = 0, shard_D = 0;
  // full mode of the batches (dkg_ceremony_batch_full_device and its primitives): ceremonies per
  // chunk of the hybrid stage (0: automatic, bfull_chunk_size)
  size_t bfull_chunk = 0;
  std::map<std::string, double> phase_ms;  // last value per "r<round>.<phase>"
};

namespace {

constexpr size_t PTB = 160;  // bytes of one extended point (40 words)
constexpr size_t PT_WORDS_H = 40;
constexpr size_t AFFP_WORDS_H = 32;  // affine addend slot of kernels.hip affine_pieces
constexpr size_t COMB_BYTES = 30 * 512 * 4;
#ifndef DKG_COMBW_BITS
#define DKG_COMBW_BITS 19
#endif
// points.h COMBW_WORDS x 4 (radix 2^19: 14 windows x 262,144 entries x 128 B = 470 MB)
constexpr size_t COMBW_BYTES =
    (size_t)(256 / DKG_COMBW_BITS + 1) * (1u << (DKG_COMBW_BITS - 1)) * 32 * 4;
const uint8_t BASEPOINT[32] = {0xe2, 0xf2, 0xae, 0x0a, 0x6a, 0xbc, 0x4e, 0x71, 0xa8, 0x84, 0xa9,
                               0x61, 0xc5, 0x00, 0x51, 0x5f, 0x58, 0xe3, 0x0b, 0x6a, 0xa5, 0x82,
                               0xdd, 0x8d, 0xb6, 0xa6, 0x59, 0x45, 0xe0, 0x8d, 0x2d, 0x76};

struct Fail {
  int code;
};

#define HCK(call)                                                                      \
  do {                                                                                 \
    hipError_t e_ = (call);                                                            \
    if (e_ != hipSuccess) {                                                            \
      ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);                    \
      throw Fail{DKG_E_DEVICE};                                                        \
    }                                                                                  \
  } while (0)

template <typename T = void>
T* buf(dkg_ctx* ctx, const char* name, size_t bytes) {
  if (bytes == 0) bytes = 16;
  auto it = ctx->bufs.find(name);
  if (it != ctx->bufs.end() && it->second.second >= bytes) return reinterpret_cast<T*>(it->second.first);
  if (it != ctx->bufs.end()) {
    HCK(hipDeviceSynchronize());  // the old buffer may still be read on any of the ctx's streams
    HCK(hipFree(it->second.first));
    ctx->bufs.erase(it);
  }
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) {
    ctx->err = std::string("hipMalloc(") + name + ", " + std::to_string(bytes) + "): " + hipGetErrorString(e);
    throw Fail{DKG_E_NOMEM};
  }
  ctx->bufs[name] = {p, bytes};
  return reinterpret_cast<T*>(p);
}

// Pinned host staging, name-keyed and grow-only like buf(): device-to-host copies into it are plain
// DMA transfers that complete with the stream, where a copy into pageable memory makes the runtime
// stage it through its own buffers on the calling thread.
template <typename T = void>
T* hbuf(dkg_ctx* ctx, const char* name, size_t bytes) {
  if (bytes == 0) bytes = 16;
  auto it = ctx->hbufs.find(name);
  if (it != ctx->hbufs.end() && it->second.second >= bytes) return reinterpret_cast<T*>(it->second.first);
  if (it != ctx->hbufs.end()) {
    HCK(hipDeviceSynchronize());  // a copy into the old buffer may still be queued
    HCK(hipHostFree(it->second.first));
    ctx->hbufs.erase(it);
  }
  void* p = nullptr;
  hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
  if (e != hipSuccess) {
    ctx->err = std::string("hipHostMalloc(") + name + ", " + std::to_string(bytes) + "): " + hipGetErrorString(e);
    throw Fail{DKG_E_NOMEM};
  }
  ctx->hbufs[name] = {p, bytes};
  return reinterpret_cast<T*>(p);
}

void h2d(dkg_ctx* ctx, void* d, const void* h, size_t n) {
  if (n) HCK(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, ctx->stream));
}
void d2h(dkg_ctx* ctx, void* h, const void* d, size_t n) {
  if (n) HCK(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, ctx->stream));
}
void sync(dkg_ctx* ctx) {
  HCK(hipStreamSynchronize(ctx->stream));
}
void check_launch(dkg_ctx* ctx) { HCK(hipGetLastError()); }

size_t pad64(size_t x) { return (x + 63) / 64 * 64; }

template <typename F>
int guarded(dkg_ctx* ctx, F&& f) {
  if (!ctx) return DKG_E_ARG;
  try {
    HCK(hipSetDevice(ctx->device));
    ctx->phase_marks.clear();  // no entry point runs inside another's guarded()
    int rc = f();
    return rc;
  } catch (const Fail& x) {
    return x.code;
  } catch (const std::exception& x) {
    ctx->err = x.what();
    return DKG_E_NOMEM;
  }
}

// The builder behind automatic mode, per kind (0 the shared bases' radix, 1 the member keys'): chained
// where it measured at least twice as fast as one thread per entry (profiles/comb_build_time.json,
// DESIGN.md section 4).
#ifndef DKG_COMBW_BUILD_AUTO
#define DKG_COMBW_BUILD_AUTO 2
#endif
#ifndef DKG_KEY_COMB_BUILD_AUTO
#define DKG_KEY_COMB_BUILD_AUTO 2
#endif
int comb_build_auto(int kind) { return kind == 0 ? DKG_COMBW_BUILD_AUTO : DKG_KEY_COMB_BUILD_AUTO; }

// The radix-2^BITS combs of the decoded points ext[.., e0 + c], c < count, into tab (kind 0: COMBW_WORDS
// words each, kind 1: key_comb_words()), by the ctx's builder; events around the launches
// (dkg_ctx_last_comb_build_ms).
void build_combs(dkg_ctx* ctx, int kind, const uint32_t* ext, size_t stride, size_t e0, uint32_t* tab,
                 hipStream_t st, size_t count) {
  const int mode = ctx->comb_build ? ctx->comb_build : comb_build_auto(kind);
  uint32_t* wbase =
      mode == 2 ? buf<uint32_t>(ctx, "cb.wbase", 4 * dkgk::comb_chain_scratch_words(kind, count)) : nullptr;
  HCK(hipEventRecord(ctx->cb_ev[0], st));
  if (mode == 2) dkgk::build_comb_chained(kind, ext, stride, e0, tab, wbase, st, count);
  else if (kind == 0) dkgk::build_combw(ext, stride, e0, tab, st, count);
  else dkgk::build_key_combs(ext, stride, e0, tab, st, count);
  HCK(hipEventRecord(ctx->cb_ev[1], st));
  ctx->last_comb_build = mode;
}

// Decode one 32-byte point and build its comb table into `tab`.
// Comb tables of one point: radix-16 (LDS kernels; may be null) and radix-2^11 (may be null).
void comb_for_point(dkg_ctx* ctx, const uint8_t p[32], uint32_t* tab, bool* ok, uint32_t* tab8 = nullptr) {
  uint32_t* comp = buf<uint32_t>(ctx, "comb_in", 32);
  uint32_t* ext = buf<uint32_t>(ctx, "comb_ext", PTB);
  uint8_t* okd = buf<uint8_t>(ctx, "comb_ok", 1);
  h2d(ctx, comp, p, 32);
  dkgk::decode_points(comp, 1, ext, 1, okd, ctx->stream);
  if (tab) dkgk::build_comb(ext, 1, 0, tab, ctx->stream);
  if (tab8) build_combs(ctx, 0, ext, 1, 0, tab8, ctx->stream, 1);
  check_launch(ctx);
  uint8_t v = 0;
  d2h(ctx, &v, okd, 1);
  sync(ctx);
  *ok = v != 0;
}

// Upload scalars (32-byte encodings) as Scalar::from_bytes reads them (from_bits, groups.rs:29-36: bit
// 255 dropped), reduced mod l.
uint32_t* upload_scalars(dkg_ctx* ctx, const char* name, const uint8_t* host, size_t count) {
  uint32_t* raw = buf<uint32_t>(ctx, "scalar_raw", 32 * count);
  uint32_t* red = buf<uint32_t>(ctx, name, 32 * count);
  h2d(ctx, raw, host, 32 * count);
  dkgk::reduce_scalars(count, raw, red, ctx->stream);
  return red;
}

// Upload an optional byte mask: null (absent) stays null.
// host words to a named device buffer; the vector is the caller's to keep until it has synchronised
uint32_t* upload_words(dkg_ctx* ctx, const char* name, const std::vector<uint32_t>& host) {
  uint32_t* d = buf<uint32_t>(ctx, name, 4 * host.size());
  h2d(ctx, d, host.data(), 4 * host.size());
  return d;
}

const uint8_t* upload_mask(dkg_ctx* ctx, const char* name, const uint8_t* host, size_t bytes) {
  if (!host) return nullptr;
  uint8_t* d = buf<uint8_t>(ctx, name, bytes);
  h2d(ctx, d, host, bytes);
  return d;
}

// Nontemporal stores for binomial step r over `columns` table columns (all chunks run their steps
// together): when the step's rows read + written, 2 (r + 1) columns 160 B, exceed DKG_BINOM_NT_BYTES
// (kernels.hip binom_pt_store).  The environment variable overrides the default for A/B runs.
// Default 0 = every step: the serialised n=1024 binomial 21.5-21.8 -> 20.4-20.6 ms, thresholds of
// 180 / 256 / 320 MB in between; config 4 and the whole ceremony within noise
// (profiles/r06_binom_levers_ab.txt, recipe r06e).
#ifndef DKG_BINOM_NT_BYTES_DEFAULT
#define DKG_BINOM_NT_BYTES_DEFAULT 0.0
#endif
bool binom_nt(size_t r, size_t columns) {
  static const double lim = [] {
    const char* e = getenv("DKG_BINOM_NT_BYTES");
    return e ? atof(e) : DKG_BINOM_NT_BYTES_DEFAULT;
  }();
  return 2.0 * (double)(r + 1) * (double)columns * 160.0 > lim;
}

// ---- the phase recorder (dkg_ctx_phase_ms): each family marks its stages with phase_mark lines and names them in
// one table of rows for phase_collect.
// The next pooled event, recorded on `st` as family `tag`'s mark closing `phase` (< 0: a start mark).  The pool
// covers the families with a fixed number of marks from dkg_ctx_create on; only the chunked loops grow it.
constexpr size_t PHASE_POOL_MIN = 32;
void phase_mark(dkg_ctx* ctx, hipStream_t st, const char* tag, int phase) {
  const size_t k = ctx->phase_marks.size();
  if (k == ctx->phase_pool.size()) {
    hipEvent_t e;
    HCK(hipEventCreate(&e));
    ctx->phase_pool.push_back(e);
  }
  HCK(hipEventRecord(ctx->phase_pool[k], st));
  ctx->phase_marks.push_back({tag, phase});
}
// ... on ctx->stream, for the families that are timed only when everything runs on that one stream
void phase_mark_serial(dkg_ctx* ctx, const char* tag, int phase) {
  if (ctx->nsub == 1) phase_mark(ctx, ctx->stream, tag, phase);
}

struct PhaseRow {
  const char* name;
  unsigned phases;  // the phase ids (bit 1 << id) whose segments the row sums
};
// After a sync: the segment between two consecutive marks of `tag` belongs to the later mark's phase (a start
// mark owns none, and marks of another tag in between cut nothing: party_round2's decrypt spans decrypt_device's
// full.* marks).  "<tag>.<name>" of every row becomes the sum of its phases' segments, over all chunks of a
// chunked loop; a row none of whose phases closed a segment did not run and is erased (reads -1).  Consumes the
// tag's marks and touches no other name.
void phase_collect(dkg_ctx* ctx, const char* tag, const PhaseRow* rows, size_t count) {
  double ms[32] = {};
  unsigned seen = 0;
  hipEvent_t prev = nullptr;
  for (size_t k = 0; k < ctx->phase_marks.size(); k++) {
    dkg_ctx::PhaseMark& m = ctx->phase_marks[k];
    if (!m.tag || strcmp(m.tag, tag)) continue;
    if (m.phase >= 0 && prev) {
      float v = 0;
      HCK(hipEventElapsedTime(&v, prev, ctx->phase_pool[k]));
      ms[m.phase] += v;
      seen |= 1u << m.phase;
    }
    prev = ctx->phase_pool[k];
    m.tag = nullptr;
  }
  for (size_t i = 0; i < count; i++) {
    const std::string name = std::string(tag) + "." + rows[i].name;
    double sum = 0;
    for (int p = 0; p < 32; p++)
      if (rows[i].phases >> p & 1) sum += ms[p];
    if (seen & rows[i].phases) ctx->phase_ms[name] = sum;
    else ctx->phase_ms.erase(name);
  }
}

// verify_device's phases under its tag r2, r4 or r24 (= fused), after the sync of a call that ran it timed; a
// verification that was not timed leaves the entries of an earlier one.
enum { VP_BINOMIAL, VP_STEPPING, VP_COMBINE, VP_CHECK };
const PhaseRow VERIFY_PHASES[] = {{"binomial", 1u << VP_BINOMIAL}, {"stepping", 1u << VP_STEPPING},
                                  {"combine", 1u << VP_COMBINE}, {"check", 1u << VP_CHECK}};
void collect_verify_phases(dkg_ctx* ctx) {
  for (const char* tag : {"r2", "r4", "r24"})
    for (const dkg_ctx::PhaseMark& m : ctx->phase_marks)
      if (m.tag && !strcmp(m.tag, tag)) {
        phase_collect(ctx, tag, VERIFY_PHASES, std::size(VERIFY_PHASES));
        break;
      }
}

// One block of rows to verify: `D` dealers [dealer_base, dealer_base + D) against receivers
// 0..n-1 in `round` (2: h*s' + g*s == sum_k j^k E_i[k]; 4: g*s == sum_k j^k A_i[k]).
// Ccomp [D][N][8] compressed commitments; s, sp [D][n][8] canonical; dec [D][n].
struct VerifySeg {
  int round;
  size_t D, dealer_base;
  const uint32_t* Ccomp;
  const uint32_t* s;
  const uint32_t* sp;
  uint8_t* dec;                       // null: no checks, the evaluations only (ctx->last_R)
  const uint8_t* extra_ok = nullptr;  // [D] device: 0 = the dealer's other broadcast data is missing
  size_t self_mod = 0;                // self = (dealer + dealer_base) mod self_mod == j; 0: n
};

// Which copy of a kernel runs a launch: product scanning (dkgk, fewer issue slots) or column sums
// (dkgk_ilp, ten independent chains per multiplication) when the launch leaves too few waves per
// SIMD to hide the serial chain (`latency_bound`), unless dkg_ctx_set_field_mode forces one.
// Binomial steps with fewer waves per SIMD than this run the column-sum copy (kernels_ilp.h).
#ifndef DKG_BINOM_PAIR_WAVES
#define DKG_BINOM_PAIR_WAVES 1.0
#endif
#ifndef DKG_BINOM_ILP_WAVES
#define DKG_BINOM_ILP_WAVES 1.5
#endif
// Product-scanning steps with fewer waves per SIMD than this run k_binom_step<.., IL> (paired
// products at a 2-wave launch bound); the environment variable DKG_BINOM_IL_WAVES overrides it (A/B).
#ifndef DKG_BINOM_IL_WAVES_DEFAULT
#define DKG_BINOM_IL_WAVES_DEFAULT 0.0
#endif
double binom_il_waves() {
  static const double v = [] {
    const char* e = getenv("DKG_BINOM_IL_WAVES");
    return e ? atof(e) : DKG_BINOM_IL_WAVES_DEFAULT;
  }();
  return v;
}
double binom_ilp_waves() {  // DKG_BINOM_ILP_WAVES, overridable the same way (A/B)
  static const double v = [] {
    const char* e = getenv("DKG_BINOM_ILP_WAVES");
    return e ? atof(e) : DKG_BINOM_ILP_WAVES;
  }();
  return v;
}
// Tables of at least this many 64-column groups (all pieces, all chunks) run the binomial as one
// launch of per-wave Horner loops (kernels.hip k_binom_wave): each wave then has a long private
// chain, and 4 rounds of a chip's resident waves keep the last round's tail small.  Fewer groups
// (n=1024: 128; n=4096: 512) keep one launch per step.
#ifndef DKG_BINOM_WAVE_PF  // the per-wave binomial's default: operands prefetched one item ahead
#define DKG_BINOM_WAVE_PF 0   // (2 waves per SIMD: config 5 +5.5 ms, profiles/r05_b5_ab.txt)
#endif
#ifndef DKG_BINOM_WAVE_DED  // the per-wave binomial with dedicated additions (+ complete redo)
#define DKG_BINOM_WAVE_DED 1
#endif
// the per-step binomial's steps without lane pairs likewise (0.5 ms on the headline, 22 ms on config
// 4, profiles/r05_binom_ded_ab.txt): in the drivers that rerun the verification with the complete
// formula when a step marked the guard word (with_binom_ded: at most twice the honest time); 2 = redo
// per wave after the last step instead (a slow worst case: a per-wave loop over a whole triangle)
#ifndef DKG_BINOM_STEP_DED
#define DKG_BINOM_STEP_DED 1
#endif
#ifndef DKG_BINOM_WAVE_COLMAJOR  // its last step writing the stepping's column-major table itself:
#define DKG_BINOM_WAVE_COLMAJOR 0  // 4-B stores 128 B apart, +10 ms against k_to_column_major's 3.3
#endif                             // (config 5, profiles/r05_b5_ab.txt)
#ifndef DKG_BINOM_WAVE_GROUPS
#define DKG_BINOM_WAVE_GROUPS 16384
#endif
#ifndef DKG_STEP_SCALED  // scaled records between the stepping and the affine normalisation (A/B: 0
#define DKG_STEP_SCALED 1  // keeps proper points and the loop's two doublings; profiles/step_scaled_ab.txt)
#endif

bool use_ilp(const dkg_ctx* ctx, bool latency_bound) {
  return ctx->fe_mode == 2 || (ctx->fe_mode == 0 && latency_bound);
}

// Work on `st` that reads the shares waits for an overlapped share evaluation (round1_device).
void wait_shares(dkg_ctx* ctx, hipStream_t st) {
  if (ctx->shares_pending) HCK(hipStreamWaitEvent(st, ctx->shares_done, 0));
}

// Coefficients held by the last of U pieces of length L (N = t + 1).  A forced split can leave the
// last pieces without any (N = 6, U = 5: L = 2, pieces 2 + 2 + 2 + 0 + 0); such a piece is a
// full-length table of identities, as are the positions past t of a ragged one.
size_t last_piece_len(size_t N, size_t U, size_t L) {
  return (U - 1) * L < N ? N - (U - 1) * L : L;
}

// Whole-column stepping slots (all U pieces of a column in one workgroup slot) when they fit and
// the launch model says so (ties to per-piece slots: more, smaller workgroups; measured on the
// 8-way n=1024 shard at U=4, 19.8 vs 20.9 ms, profiles/r02_shard_stepping_ab.txt).
bool stepping_whole_pays(size_t cols, size_t U, size_t L, size_t Lr) {
  return dkgk::stepping_whole_columns(L, U, Lr) &&
         dkgk::stepping_cycles(cols, L, U, Lr, true) < 0.98 * dkgk::stepping_cycles(cols, L, U, Lr, false);
}

// ---- degree split ----
// P(x) = sum_{u<U} x^(uL) Q_u(x), deg Q_u < L = ceil(N / U): the binomial-basis Horner runs on the
// U pieces (quadratic in the degree: ~1/U of the work, and ~1/U of the dependent chain), the
// stepping does the same number of additions, and one recombination per (column, receiver) adds
// U-1 multiplications by y_j = j^L mod l (k_combine).  Split when that is cheaper.
// Instruction-count model of binomial + stepping + recombination (static VALU counts of the
// kernels; the check does not depend on U) in SIMD
// cycles: a SIMD retires one wave instruction per ~4.5 cycles of this mix when it has >= 2 waves,
// one per ~8 when a lone wave runs a dependent chain (tools/ubench/ilp.hip); 1024 SIMDs.
// Short multipliers are implemented up to this many pieces (k_combine_aff's digit words; the
// projective-addend k_combine_short stops at 4)
constexpr size_t SHORT_MAX = 5;
#ifndef DKG_AUTO_SHORT5
#define DKG_AUTO_SHORT5 0
#endif

// short_mult: 0 powers of y, 1 short multipliers as per-scalar NAFs, 2 pairwise JSF where built
constexpr int SM_POWERS = 0, SM_NAF = 1, SM_JSF = 2;
bool jsf_built(size_t U) { return U == 2 || U == 4; }  // k_combine_jsf

double split_model_ms(size_t cols, size_t n, size_t N, size_t U, size_t L, int short_mult) {
  const double DBL = 1000, ADD = 1400, SIMDS = 1024, THR = 4.5, LAT = 8, LAT_ILP = 6, LAUNCH = 3e-3 * 2.4e6;
  const size_t Lr = last_piece_len(N, U, L), off = L - Lr;  // the last piece: Lr positions, starts at step off
  auto cost = [&](size_t m) {  // one binomial position-step: add + multiplication by m
    // length and weight of m's recoding as the kernels do it (points.h small_recode: the NAF, a
    // leading 1 0 -1 turned into 1 1 -- one doubling fewer)
    uint64_t pos = 0, neg = 0;
    int len = 0;
    for (uint64_t v = m; v; v >>= 1, len++) {
      if (v & 1) {
        if ((v & 3) == 1) {
          pos |= 1ull << len;
          v -= 1;
        } else {
          neg |= 1ull << len;
          v += 1;
        }
      }
    }
    if (len >= 3 && !(((pos | neg) >> (len - 2)) & 1) && ((neg >> (len - 3)) & 1)) {
      pos = (pos & ~(1ull << (len - 1))) | (3ull << (len - 3));
      neg &= ~(1ull << (len - 3));
      len--;
    }
    const int nz = __builtin_popcountll(pos | neg);
    return ADD + (len > 1 ? (len - 1) * DBL + (nz - 1) * ADD : 0.0);
  };

  std::vector<double> pre(L + 1, 0.0);
  for (size_t m = 1; m <= L; m++) pre[m] = pre[m - 1] + cost(m);
  const double waves_col = (double)cols / 64;
  double cyc = 0;
  for (size_t r = 1; r < L; r++) {
    // wave-instructions of step r: U-1 full pieces, the last one from step off on
    const double work = waves_col * ((U - 1) * pre[r] + (r > off ? pre[r - off] : 0.0)) * THR / SIMDS;
    // a step pays its issue work AND its longest chain: the last waves of a launch run their chains
    // on partly idle SIMDs (the sum fits the measured shards within 5 %: 1-, 2-, 4-, 8-way n=1024,
    // one-GPU n=4096; the max alone picked U=2 for a 4-way n=1024 shard, 3 % slower than U=4).
    // Steps with under 1.5 waves per SIMD run the column-sum copy (verify_device), whose ten
    // independent chains per multiplication shorten the latency-bound chain (8-way n=1024 shard:
    // binomial 6.78 -> 6.26 ms at U=3, profiles/r02_shard_stepping_ab.txt).
    const double lat = waves_col * U * (r + 1) / SIMDS < 1.5 ? LAT_ILP : LAT;
    cyc += work + cost(r) * lat + LAUNCH;
  }
  if (U > 1) {
    // short multipliers (U <= 4): one joint chain of 253 (U-1)/U doublings over U NAFs of that
    // length (~1/3 nonzero); powers of y: pairwise joint chains, an even U starting with one
    // product (253 doublings + ~85 NAF additions), then (ceil(U/2) - 1) joint y^2 / y steps (253
    // doublings + ~170 additions)
    // pairwise JSF (U = 2, 4): a pair's joint form has every second column nonzero, a leftover
    // piece's NAF every third; a pair's four addends cost 39 products (k_affine_pairs) against the
    // 15.5 of its two pieces alone (k_affine_pieces): ~11.75 of an addition's 8 per sum or difference
    const double bits = 253.0 * (U - 1) / U;
    const bool jsf = short_mult == SM_JSF && jsf_built(U);
    const double adds = jsf ? (U / 2) * bits / 2 + (U % 2) * bits / 3 : U * bits / 3;
    const double per = short_mult && U <= SHORT_MAX ? bits * 950 + adds * ADD + (jsf ? 2 * (U / 2) * 11.75 / 8 * ADD : 0.0)
                                            : (U % 2 == 0 ? 253 * 950 + 85 * ADD : 0.0) +
                                                  ((U + 1) / 2 - 1) * (253 * 950 + 170 * ADD);
    const double waves = (double)cols / 64 * n;
    cyc += std::max(waves * per * THR / SIMDS, per * LAT);  // the 2-slot variant runs at 2 waves/SIMD as fast
  }
  // stepping: n dependent additions per lane, in the launches k_stepping gets (dkgk::stepping_cycles)
  // (less the wave-steps of waves whose positions are all dead: the banded lane map, step_map.h)
  cyc += n * ADD * dkgk::stepping_cycles(cols, L, U, Lr, stepping_whole_pays(cols, U, L, Lr), n);
  return cyc / 2.4e6;
}

// Piece length of a U-way split: ceil(N / U), or that rounded up to a multiple of 64 when the
// model prefers it -- whole 64-lane waves for the stepping's per-piece tables and a shorter last
// piece (N = 550, U = 2: 320 + 230 instead of 275 + 275, two tables of 5 and 4 waves instead of
// 5 + 5 with 45 idle lanes each).  When all pieces of a column fit one stepping workgroup
// (N <= 512) ceil(N / U) always wins: N = 512, U = 3 runs 171 + 171 + 170 on 512 lanes.
size_t split_len(size_t cols, size_t n, size_t N, size_t U, int short_mult = SM_JSF) {
  const size_t L1 = (N + U - 1) / U;
  if (U == 1) return L1;
  const size_t L64 = (L1 + 63) / 64 * 64;
  if (L64 == L1 || (U - 1) * L64 >= N) return L1;
  return split_model_ms(cols, n, N, U, L64, short_mult) < split_model_ms(cols, n, N, U, L1, short_mult) ? L64 : L1;
}

double split_model_ms(size_t cols, size_t n, size_t N, size_t U, int short_mult = SM_JSF) {
  return split_model_ms(cols, n, N, U, split_len(cols, n, N, U, short_mult), short_mult);
}

// the recombination the context's settings select (JSF needs the affine addends' planes)
int short_kind(const dkg_ctx* ctx) {
  if (ctx->combine_mode == 1) return SM_POWERS;
  return ctx->combine_mode == 3 || ctx->addend_mode != 0 ? SM_NAF : SM_JSF;
}

size_t choose_split(dkg_ctx* ctx, size_t cols, size_t n, size_t N) {
  if (ctx->split > 0) return std::min<size_t>((size_t)ctx->split, N);
  const int sm = short_kind(ctx);
  const double base = split_model_ms(cols, n, N, 1, sm);
  std::vector<double> ms(17, 0.0);
  double best_ms = base;
  size_t umax = 1;
  for (size_t U = 2; U <= 16; U++) {
    if (N < 64 * U) break;  // pieces of degree < 63: the binomial is cheap already
    // five-piece short multipliers are priced for the automatic choice only with DKG_AUTO_SHORT5:
    // they are parity-tested (forced splits) but their shard timings are unmeasured, so by default
    // the model ranks U = 5 with powers as before (it then never wins) -- dkg_ctx_set_split(5)
    // runs them
    ms[U] = split_model_ms(cols, n, N, U, U <= 4 || (ctx->addend_mode == 0 && DKG_AUTO_SHORT5) ? sm : SM_POWERS);
    best_ms = std::min(best_ms, ms[U]);
    umax = U;
  }
  if (!(best_ms < 0.9 * base)) return 1;  // only for a clear win
  // the model's best (with short multipliers it ranks the measured n=1024 shards right: U=4 ahead
  // of U=3 by 0.3-0.5 ms per rank at 1-8 ranks, U=5 -- powers of y again -- far behind;
  // profiles/r02_lattice_ab.txt)
  for (size_t U = 2; U <= umax; U++)
    if (ms[U] <= best_ms) return U;
  return 1;
}

// NAF of y = (j+1)^L mod l and of y^2 for receivers j = 0..n-1 (k_combine's wave-uniform
// multipliers), cached per (n, L) on the device: digits [n][2][256] int8, top [n][2] int16.
void naf_digits(const uint8_t b[32], int8_t* d, int16_t* tp) {
  uint32_t k[9] = {0};
  for (int w = 0; w < 8; w++)
    k[w] = (uint32_t)b[4 * w] | (uint32_t)b[4 * w + 1] << 8 | (uint32_t)b[4 * w + 2] << 16 | (uint32_t)b[4 * w + 3] << 24;
  *tp = -1;
  for (int i = 0; i < 256; i++) {  // k < 2^253: the NAF fits in 254 digits
    d[i] = 0;
    if (!((k[i >> 5] >> (i & 31)) & 1u)) continue;
    int8_t dg = 1;
    if ((k[(i + 1) >> 5] >> ((i + 1) & 31)) & 1u) {  // ...11: digit -1, k += 2^i
      dg = -1;
      uint64_t carry = 1ull << (i & 31);
      for (int w = i >> 5; carry && w < 9; w++) {
        const uint64_t sum = (uint64_t)k[w] + carry;
        k[w] = (uint32_t)sum;
        carry = sum >> 32;
      }
    } else {
      k[i >> 5] &= ~(1u << (i & 31));
    }
    d[i] = dg;
    *tp = (int16_t)i;
  }
}

void split_digits(dkg_ctx* ctx, size_t n, size_t L, const int8_t** digits, const int16_t** top) {
  int8_t* dd = buf<int8_t>(ctx, "v.ydig", 512 * n);
  int16_t* dt = buf<int16_t>(ctx, "v.ytop", 4 * n);
  *digits = dd;
  *top = dt;
  if (ctx->ydig_n == n && ctx->ydig_L == L) return;
  std::vector<int8_t> hd(512 * n, 0);
  std::vector<int16_t> ht(2 * n, -1);
  for (size_t j = 0; j < n; j++) {
    dkgh::Zl x = dkgh::zl_from_u64(j + 1), y = dkgh::zl_from_u64(1);
    for (size_t e = L; e; e >>= 1) {  // y = x^L
      if (e & 1) y = dkgh::zl_mul(y, x);
      x = dkgh::zl_mul(x, x);
    }
    uint8_t b[32];
    dkgh::zl_to_bytes(b, y);
    naf_digits(b, &hd[512 * j], &ht[2 * j]);
    dkgh::zl_to_bytes(b, dkgh::zl_mul(y, y));
    naf_digits(b, &hd[512 * j + 256], &ht[2 * j + 1]);
  }
  h2d(ctx, dd, hd.data(), hd.size());
  h2d(ctx, dt, ht.data(), 4 * n);
  ctx->ydig_n = n;
  ctx->ydig_L = L;
}

// Short recombination multipliers (lattice.cpp) of receivers j = 1..n for a K-way split, K <= 4
// (k_combine_short): digits [n][256] u32, byte u of word b = the signed NAF digit at position b of
// the scalar of piece u; top [n] int16 = the highest position with a nonzero digit; scale [n][8]
// words = b_j 2^256 mod l, the checks' Montgomery factor taking s to b_j s.  Cached per (n, L, K, recoding).
// (one LLL per receiver, ~1 ms at K = 4: spread over up to 16 host threads)
void short_vectors(size_t n, size_t L, size_t K, std::vector<uint8_t>& mag, std::vector<int8_t>& sign, bool jsf) {
  mag.assign(n * K * 32, 0);
  sign.assign(n * K, 1);
  auto rows = [&](size_t j0, size_t j1) {
    for (size_t j = j0; j < j1; j++) {
      dkgh::Zl x = dkgh::zl_from_u64(j + 1), y = dkgh::zl_from_u64(1);
      for (size_t e = L; e; e >>= 1) {  // y = x^L
        if (e & 1) y = dkgh::zl_mul(y, x);
        x = dkgh::zl_mul(x, x);
      }
      dkgh::short_multipliers(y, (int)K, reinterpret_cast<uint8_t(*)[32]>(&mag[j * K * 32]), &sign[j * K], jsf);
    }
  };
  const size_t nt = std::min<size_t>({(size_t)std::max(1u, std::thread::hardware_concurrency()), 16, (n + 63) / 64});
  std::vector<std::thread> th;
  for (size_t i = 1; i < nt; i++) th.emplace_back(rows, n * i / nt, n * (i + 1) / nt);
  rows(0, n / nt);
  for (auto& t : th) t.join();
}

// The chain's digit words for the rows (mag, sign) of short_vectors: hd [2][n][256] (word 0: pieces
// 0..3, word 1: 4..), ht [n].  jsf: pairs (0,1) and (2,3) are recoded jointly in Solinas' joint
// sparse form (magnitudes first, then each scalar's sign on its digits), a leftover piece keeps its
// NAF; hev [n][JSF_EV_WORDS] then lists the pair-sum plane and sign of every both-nonzero column in
// chain order (kernels_decl.inc combine_short_jsf).  A JSF may be one position longer than the NAF:
// entries are below 2^253, so 256 positions hold it.
bool short_digit_words(size_t n, size_t K, bool jsf, const std::vector<uint8_t>& mag, const std::vector<int8_t>& sign,
                       std::vector<uint32_t>& hd, std::vector<int16_t>& ht, std::vector<uint32_t>* hev) {
  hd.assign(2 * 256 * n, 0);
  ht.assign(n, -1);
  if (hev) hev->assign(dkgk::JSF_EV_WORDS * n, dkgk::JSF_EV_NONE);
  for (size_t j = 0; j < n; j++) {
    auto put = [&](size_t u, const int8_t* d) {
      for (int b = 0; b < 256; b++)
        hd[(u / 4) * 256 * n + 256 * j + b] |= (uint32_t)(uint8_t)(int8_t)(d[b] * sign[j * K + u]) << (8 * (u % 4));
    };
    for (size_t u = 0; u < K; u++) {
      int8_t d[256], d1[256];
      int16_t tp;
      if (jsf && u + 1 < K) {
        if (!dkgh::jsf_digits(&mag[(j * K + u) * 32], &mag[(j * K + u + 1) * 32], d, d1, &tp)) return false;
        put(u, d);
        put(u + 1, d1);
        u++;
      } else {
        naf_digits(&mag[(j * K + u) * 32], d, &tp);
        put(u, d);
      }
      ht[j] = std::max(ht[j], tp);
    }
    if (jsf && hev) {
      size_t k = 0;
      for (int b = ht[j]; b >= 0; b--) {
        const uint32_t w = hd[256 * j + b];
        for (size_t p = 0; p < K / 2 && p < 2; p++) {
          const int e0 = (int8_t)(w >> (16 * p)), e1 = (int8_t)(w >> (16 * p + 8));
          if (!e0 || !e1) continue;
          if (k + 2 >= dkgk::JSF_EV_WORDS) return false;  // never for a JSF (<= 2/3 of the columns)
          (*hev)[dkgk::JSF_EV_WORDS * j + k++] = (uint32_t)(2 * p + (e0 != e1) + (e0 < 0 ? 4 : 0));
        }
      }
    }
  }
  return true;
}

void split_short(dkg_ctx* ctx, size_t n, size_t L, size_t K, bool jsf, const uint32_t** digits, const int16_t** top,
                 const uint32_t** scale, const uint32_t** events) {
  uint32_t* dd = buf<uint32_t>(ctx, "v.sdig", 2 * 4 * 256 * n);  // word 0: pieces 0..3, word 1: 4..
  int16_t* dt = buf<int16_t>(ctx, "v.stop", 2 * n);
  uint32_t* ds = buf<uint32_t>(ctx, "v.sscale", 32 * n);
  uint32_t* de = buf<uint32_t>(ctx, "v.sev", 4 * dkgk::JSF_EV_WORDS * n);
  *digits = dd;
  *top = dt;
  *scale = ds;
  *events = de;
  if (ctx->sdig_n == n && ctx->sdig_L == L && ctx->sdig_K == K && ctx->sdig_jsf == (int)jsf) return;
  std::vector<uint8_t> mag;
  std::vector<int8_t> sign;
  short_vectors(n, L, K, mag, sign, jsf);
  std::vector<uint32_t> hd, hs(8 * n, 0), hev;
  std::vector<int16_t> ht;
  if (!short_digit_words(n, K, jsf, mag, sign, hd, ht, &hev)) {
    ctx->err = "split_short: a joint sparse form does not fit its digit words";
    throw Fail{DKG_E_ARG};
  }
  uint8_t r256[33] = {0};
  r256[32] = 1;
  const dkgh::Zl R = dkgh::zl_from_bytes_wide(r256, 33);  // 2^256 mod l
  for (size_t j = 0; j < n; j++) {
    const dkgh::Zl b = dkgh::zl_from_bytes_wide(&mag[j * K * 32], 32);  // b > 0
    uint8_t w[32];
    dkgh::zl_to_bytes(w, dkgh::zl_mul(b, R));
    memcpy(&hs[8 * j], w, 32);
  }
  ctx->sdig_jsf = -1;  // the key holds only once every copy is queued
  h2d(ctx, dd, hd.data(), 4 * hd.size());
  h2d(ctx, dt, ht.data(), 2 * n);
  h2d(ctx, ds, hs.data(), 4 * hs.size());
  h2d(ctx, de, hev.data(), 4 * hev.size());
  ctx->sdig_n = n;
  ctx->sdig_L = L;
  ctx->sdig_K = K;
  ctx->sdig_jsf = (int)jsf;
}

// One or two segments on device, as ONE pipeline over "virtual dealers" (table columns).  With two
// segments (round 2 on E and round 4 on A of the SAME dealers) a dealer's E row and A row are two
// independent polynomials in the exponent: the binomial-basis Horner and the stepping never look
// at which one a column is, so both run in the same launches (twice the independent work inside
// each of the t dependent binomial launches, half the launches).  Columns are interleaved in
// 64-dealer groups (E of dealers 64q.., then A of the same dealers) so that a chunk holds both rows
// of its dealers and one fused check computes g*s_ij once for both rounds.  Work is ordered after
// what is queued on ctx->stream and completes on it.  With ctx->nsub > 1 the dealer groups are cut
// into nsub chunks whose binomial -> stepping -> check pipelines run on their own streams, so one
// chunk's partly-filled binomial launches share the CUs with another chunk's work.  nsub == 1
// with `timed` records per-phase device times (dkg_ctx_phase_ms, under `tag`).
void verify_device(dkg_ctx* ctx, size_t n, size_t t, const VerifySeg* segs, int nseg, bool timed,
                   const char* tag) {
  const size_t N = t + 1, D = segs[0].D;
  if (!D) return;
  if (nseg == 2 && (segs[1].D != D || segs[1].dealer_base != segs[0].dealer_base || segs[1].s != segs[0].s ||
                    segs[0].round != 2 || segs[1].round != 4)) {
    ctx->err = "verify_device: fused segments must be round 2 then round 4 of the same dealers";
    throw Fail{DKG_E_ARG};
  }
  const size_t groups = (D + 63) / 64, gw = 64 * nseg;  // columns per dealer group
  const size_t npad = groups * gw;
  // degree split: U pieces of L positions; piece u of column c is table column u * npad + c
  const size_t U = choose_split(ctx, npad, n, N), L = split_len(npad, n, N, U, short_kind(ctx)), W = U * npad;
  const size_t Lr = last_piece_len(N, U, L);  // the last piece's length (L or shorter)
  const bool whole = ctx->step_mode == 1 || ((ctx->step_mode == 0 || ctx->step_mode == 3) && stepping_whole_pays(npad, U, L, Lr));
  // the stepping keeps product scanning even at 2 waves per SIMD (8-way n=1024 shard, one stream:
  // 6.07 vs 6.12 ms with column sums, profiles/r02_shard_stepping_ab.txt); only a forced mode 2
  // switches it
  const bool step_ilp = use_ilp(ctx, false);
  ctx->last_split = (int)U;
  ctx->last_split_len = L;
  hipStream_t home = ctx->stream;
  uint8_t* pok = buf<uint8_t>(ctx, "v.pok", npad * N);
  uint8_t* dok = buf<uint8_t>(ctx, "v.dok", npad);
  uint32_t* Cpm = buf<uint32_t>(ctx, "v.Cpm", PTB * L * W);
  uint32_t* e0 = buf<uint32_t>(ctx, "v.binom0", PTB * L * W);
  uint32_t* e1 = buf<uint32_t>(ctx, "v.binom1", PTB * L * W);
  uint32_t* eT = buf<uint32_t>(ctx, "v.binomT", PTB * L * W);  // column-major copy for the stepping
  // short multipliers up to SHORT_MAX pieces with affine addends, 4 with projective ones
  const bool short_mult = U > 1 && U <= (ctx->addend_mode == 0 ? SHORT_MAX : 4) && ctx->combine_mode != 1;
  // pairwise JSF chains: the pairs' sums and differences are 2 floor(U/2) more piece planes of Aff
  // after the U stepped ones (the chunk offsets do not change); R holds the stepped ones only
  // (k_combine_jsf keeps a lane's column * n in 32 bits: any table that fits device memory)
  const bool jsf = short_mult && short_kind(ctx) == SM_JSF && jsf_built(U) && (uint64_t)npad * n < (1ull << 32);
  const size_t WP = jsf ? (U + 2 * (U / 2)) * npad : W;
  uint32_t* R = buf<uint32_t>(ctx, "v.R", PTB * W * n);
  uint32_t *sa = nullptr, *sb = nullptr;
  if (L > 512) {
    sa = buf<uint32_t>(ctx, "v.step_a", PTB * W * n);
    sb = buf<uint32_t>(ctx, "v.step_b", PTB * W * n);
  }
  const int8_t* ydig = nullptr;
  const int16_t* ytop = nullptr;
  const uint32_t *sdig = nullptr, *sscale = nullptr, *sev = nullptr;  // short multipliers: R holds b_j P(j)
  const int16_t* stop = nullptr;
  // stepping flags of the dedicated additions: chunk c0's words start at stepping_flag_words(c0, U)
  uint32_t* sflags = ctx->step_formula == 0
                         ? buf<uint32_t>(ctx, "v.sflags", 4 * dkgk::stepping_flag_words(npad, U)) : nullptr;
  ctx->last_step_flags = sflags;
  ctx->last_step_flag_words = sflags ? dkgk::stepping_flag_words(npad, U) : 0;
  // affine addends: one 128-B slot per (piece column, receiver), like R
  uint32_t* Aff = short_mult && ctx->addend_mode == 0 ? buf<uint32_t>(ctx, "v.Aff", 4 * AFFP_WORDS_H * WP * n) : nullptr;
  // the stepping's dense copy of each stored point's Z (40 B), read by the affine normalisation
  // (k_affine_pieces; the JSF chains' k_affine_pairs reads Z and T from R, so there is none)
  uint32_t* Rz = Aff && !jsf ? buf<uint32_t>(ctx, "v.Rz", 40 * W * n) : nullptr;
  // the stepped values' one reader is the affine normalisation: the stepping leaves scaled records
  // (kernels.hip k_stepping SC: no doublings in its loop) and the normalisation folds the constants.
  // Every other reader of the stepped R (k_combine*, the checks at U = 1) takes proper points.
  const bool r_scaled = DKG_STEP_SCALED && Aff != nullptr;
  if (short_mult) split_short(ctx, n, L, U, jsf, &sdig, &stop, &sscale, &sev);
  else if (U > 1) split_digits(ctx, n, L, &ydig, &ytop);
  ctx->last_combine = U > 1 ? (short_mult ? 2 : 1) : 0;
  ctx->last_R = R;
  ctx->last_scale = sscale;
  ctx->last_dok = dok;
  ctx->last_dok_nseg = nseg;
  ctx->last_pok = pok;
  ctx->last_npad = npad;
  // padding columns, and the positions past t of the last piece, are the identity
  if (npad != D * nseg || U * L != N) dkgk::fill_identity(L * W, Cpm, home);
  HCK(hipMemsetAsync(pok, 1, npad * N, home));
  // deferred round 1 (BatchRound1): the fused pass over the very dealers whose coefficients wait
  const bool defer_r1 = ctx->r1_a && nseg == 2 && D == ctx->r1_D;
  for (int k = 0; k < nseg && !defer_r1; k++) {
    const uint32_t* ext = segs[k].round == 2 ? ctx->ext_E : ctx->ext_A;
    if (ext)  // generated on this device: group elements, as the reference's broadcasts carry them
      dkgk::place_position_major(ext, ctx->ext_stride, D, N, W, Cpm, home, nseg, k, L, npad);
    else  // K5 (groups.rs:78-81) into the position-major table
      dkgk::decode_position_major(segs[k].Ccomp, D, N, W, Cpm, pok, home, nseg, k, L, npad);
  }
  dkgk::dealer_ok(npad, N, pok, dok, home);
  // an extra mask produced by the overlapped decryption (full mode) is applied by each chunk's
  // checks once the shares are there; otherwise here
  const bool defer_masks = ctx->shares_pending;
  for (int k = 0; k < nseg; k++)
    if (segs[k].extra_ok && !defer_masks) dkgk::and_dealer_mask(D, nseg, k, segs[k].extra_ok, dok, home);
  // checks of dealers [d0, d1) on stream st
  auto checks = [&](size_t d0, size_t d1, hipStream_t st, size_t j0 = 0, size_t jn = 0) {
    if (d1 <= d0 || !segs[0].dec) return;
    wait_shares(ctx, st);
    if (defer_masks)  // dealers [d0, d1) start a column group (d0 = 64 g0): relative indexing
      for (int k = 0; k < nseg; k++)
        if (segs[k].extra_ok) dkgk::and_dealer_mask(d1 - d0, nseg, k, segs[k].extra_ok + d0, dok + d0 * nseg, st);
    const VerifySeg& g = segs[0];
    if (nseg == 2) {
      // split combs: every chunk parks its pairs' g*s at its own dealers' offset
      uint32_t* acc = ctx->check_mode == 1 ? buf<uint32_t>(ctx, "v.acc", PTB * D * n) + d0 * n * PT_WORDS_H : nullptr;
      dkgk::check_both(d1 - d0, n, d0, g.dealer_base, g.self_mod ? g.self_mod : n, g.s, g.sp, R,
                       ctx->tab_gw, ctx->tab_hw, dok, g.dec, segs[1].dec, st, sscale, j0, jn, acc);
    } else {
      dkgk::check(d1 - d0, n, g.dealer_base + d0, 0, g.self_mod ? g.self_mod : n, g.round, g.s + d0 * n * 8,
                  g.round == 2 ? g.sp + d0 * n * 8 : nullptr, R + d0 * n * PT_WORDS_H, ctx->tab_gw, ctx->tab_hw,
                  dok + d0, g.dec + d0 * n, st, sscale);
    }
  };
  // dealer groups [g0, g1) = columns [g0 * gw, g1 * gw)
  // Chunk streams pay when the binomial saturates the GPU (chunk c+1's triangle fills the CUs that
  // chunk c's launch tails leave idle), or when the stepping is long enough (W * L * n lane-steps)
  // that the chunks' phases drift apart and one chunk's recombination and checks run beside the
  // other's stepping.  A small ceremony or shard is latency-bound -- every binomial step is one
  // dependent NAF chain long whatever its width -- and two half-width pipelines only double its
  // launches.  Measured (tools/shard_time.py): chunks gain 1.2-2.4 ms on n=512 1- and 2-way (>= 6.7e7
  // lane-steps) and 0.3-0.8 ms on n=1024 1- to 4-way, and lose 0.9-2.5 ms on n=512 4-way and n=256
  // (<= 3.4e7) -- and 2 ms on the 8-way n=1024 shard (256 columns: two half-width stepping launches
  // of 128 workgroups each, 18.1 vs 20.2 ms, profiles/r02_shard_stepping_ab.txt), so a long stepping
  // needs at least 512 columns too.
  const bool saturating = (W / 64) * (L / 2) >= 4 * 1024;
  const bool long_stepping = (double)W * (double)L * (double)n >= 5e7 && npad >= 512;
  const size_t nsub = (saturating || long_stepping) ? std::min<size_t>(ctx->nsub, groups) : 1;
  // the binomial as per-wave Horner loops (k_binom_wave) for tables of many column groups
  const bool per_wave = ctx->binom_mode == 4 || ctx->binom_mode == 5 ||
                        (ctx->binom_mode == 0 && L > 1 && (double)npad / 64 * U >= DKG_BINOM_WAVE_GROUPS);
  ctx->last_binomial = per_wave ? 1 : 0;
  // the per-wave binomial's dedicated additions (with the stepping's formula setting): one redo flag
  // per (piece, 64-column group), zeroed before the chunks fork
  // (and of the per-step binomial's steps without lane pairs under DKG_BINOM_STEP_DED=2, redone per
  // wave; =1 marks the one guard word of with_binom_ded instead)
  uint32_t* bflags = nullptr;
  const bool wave_ded = per_wave && DKG_BINOM_WAVE_DED && ctx->binom_mode != 5 &&
                        !(ctx->binom_mode == 0 && DKG_BINOM_WAVE_PF);
  const bool step_ded = !per_wave && ((DKG_BINOM_STEP_DED == 1 && ctx->binom_step_ded && ctx->binom_any) ||
                                      DKG_BINOM_STEP_DED == 2);
  if (ctx->step_formula == 0 && (wave_ded || (step_ded && DKG_BINOM_STEP_DED == 2))) {
    bflags = buf<uint32_t>(ctx, "v.bflags", 4 * (W / 64));
    HCK(hipMemsetAsync(bflags, 0, 4 * (W / 64), home));
  }
  ctx->last_bflags = bflags;
  ctx->last_bflag_words = bflags ? W / 64 : 0;
  // the rerun guard's word (with_binom_ded): zeroed when the verification began (verify_rounds)
  uint32_t* bany = step_ded && DKG_BINOM_STEP_DED == 1 && ctx->step_formula == 0 ? ctx->binom_any : nullptr;
  // dead-position repack of an unsplit table (kernels.hip stepping_tail_phases): two scratch states
  const bool tails = ctx->step_mode != 3 && dkgk::stepping_tail_phases(L, n, U) > 1;
  uint32_t* tail_a = tails ? buf<uint32_t>(ctx, "v.tail_a", 4 * dkgk::stepping_tail_words(npad, L)) : nullptr;
  uint32_t* tail_b = tails ? buf<uint32_t>(ctx, "v.tail_b", 4 * dkgk::stepping_tail_words(npad, L)) : nullptr;
  auto chunk = [&](size_t g0, size_t g1, hipStream_t st, bool tm) {
    const size_t c0 = g0 * gw, w = (g1 - g0) * gw;
    if (defer_r1) {  // this chunk's dealers' commitments (committee.rs:151-159), into their columns
      const size_t d0 = g0 * 64, d1 = std::min(D, g1 * 64);
      dkgk::commit_position_major(d1 - d0, N, ctx->r1_a + d0 * N * 8, ctx->r1_b + d0 * N * 8, ctx->tab_gw,
                                  ctx->tab_hw, Cpm + c0, W, L, npad, ctx->r1_A0 + d0, D, st);
    }
    if (tm) phase_mark(ctx, st, tag, -1);
    const uint32_t* e;
    if (per_wave) {
      e = dkgk::binomial_wave(w, W, L, Cpm + c0, e0 + c0, st, U, npad, Lr,
                              DKG_BINOM_WAVE_COLMAJOR ? eT + c0 * L : nullptr,
                              ctx->binom_mode == 5 || (ctx->binom_mode == 0 && DKG_BINOM_WAVE_PF), bflags, c0, D,
                              (unsigned)gw);
    } else {
      dkgk::binom_init(w, W, L, Cpm + c0, e0 + c0, st, U, npad);
      uint32_t *bin = e0 + c0, *bout = e1 + c0;
      for (size_t r = 1; r < L; r++) {
        // step r has (r + 1) waves per 64 columns and piece, over all chunks at once
        const double wps = (double)npad / 64 * U * (r + 1) / 1024;  // waves per SIMD, all chunks
        const bool ilp = use_ilp(ctx, wps < binom_ilp_waves());
        // lane pairs (k_binom_pair): by default the steps with under one wave per SIMD, mode 2
        // every step (1-, 2-, 4-, 8-way n=1024 shards 0.2-0.4 ms faster;
        // profiles/r03_binomial_pairs_ab.txt)
        const bool pair = ctx->binom_mode == 2 || ((ctx->binom_mode == 0 || ctx->binom_mode == 3) &&
                                                   wps < DKG_BINOM_PAIR_WAVES);
        if (pair)
          (ilp ? dkgk_ilp::binom_step_pair : dkgk::binom_step_pair)(r, w, W, L, Cpm + c0, bin, bout, st, U, npad,
                                                                    Lr);
        else
          (ilp ? dkgk_ilp::binom_step : dkgk::binom_step)(r, w, W, L, Cpm + c0, bin, bout, st, U, npad, Lr,
                                                          bany ? bany : bflags, c0, D, (unsigned)gw, bany != nullptr,
                                                          binom_nt(r, npad * U), !ilp && wps < binom_il_waves());
        std::swap(bin, bout);
      }
      e = bin;
      if (bflags && DKG_BINOM_STEP_DED == 2)
        dkgk::binomial_wave_redo(w, W, L, Cpm + c0, bin, st, U, npad, Lr, bflags, c0, D, (unsigned)gw);
    }
    if (tm) phase_mark(ctx, st, tag, VP_BINOMIAL);
    if (!per_wave || !DKG_BINOM_WAVE_COLMAJOR)  // timed with the stepping
      dkgk::to_column_major(w, W, L, e, eT + c0 * L, U, npad, st);
    uint32_t* fl = sflags ? sflags + dkgk::stepping_flag_words(c0, U) : nullptr;
    if (fl) HCK(hipMemsetAsync(fl, 0, 4 * dkgk::stepping_flag_words(w, U), st));
    auto step = step_ilp ? dkgk_ilp::stepping : dkgk::stepping;
    if (!step(w, W, L, eT + c0 * L, n, R + c0 * n * PT_WORDS_H, sa ? sa + c0 * n * 40 : nullptr,
              sb ? sb + c0 * n * 40 : nullptr, st, U, npad, Lr, whole, fl, c0, D, (unsigned)gw,
              Rz ? Rz + c0 * n * 10 : nullptr, tail_a, tail_b, r_scaled))
      throw Fail{DKG_E_ARG};  // stepping flag words: an internal layout error, never silently dropped
    if (tm) phase_mark(ctx, st, tag, VP_STEPPING);
    if (jsf) {
      dkgk::affine_pairs(w, npad, U, n, R + c0 * n * PT_WORDS_H, Aff + c0 * n * AFFP_WORDS_H, st, 0, 0, r_scaled);
      dkgk::combine_short_jsf(w, npad, U, n, sdig, stop, sev, Aff + c0 * n * AFFP_WORDS_H, R + c0 * n * PT_WORDS_H, st);
    } else if (short_mult && Aff) {
      dkgk::affine_pieces(w, npad, U, n, R + c0 * n * PT_WORDS_H, Aff + c0 * n * AFFP_WORDS_H, st, Rz + c0 * n * 10, 0,
                          0, r_scaled);
      dkgk::combine_short_aff(w, npad, U, n, sdig, stop, Aff + c0 * n * AFFP_WORDS_H, R + c0 * n * PT_WORDS_H, st);
    } else if (short_mult) dkgk::combine_short(w, npad, U, n, sdig, stop, R + c0 * n * PT_WORDS_H, st);
    else dkgk::combine(w, npad, U, n, ydig, ytop, R + c0 * n * PT_WORDS_H, st);
    if (tm) phase_mark(ctx, st, tag, VP_COMBINE);
    checks(g0 * 64, std::min(D, g1 * 64), st);
    if (tm) phase_mark(ctx, st, tag, VP_CHECK);
  };
  if (nsub <= 1) {
    chunk(0, groups, home, timed);
  } else {
    HCK(hipEventRecord(ctx->fork, home));
    size_t g0 = 0;
    for (size_t c = 0; c < nsub; c++) {
      const size_t g1 = groups * (c + 1) / nsub;
      HCK(hipStreamWaitEvent(ctx->sub[c], ctx->fork, 0));
      chunk(g0, g1, ctx->sub[c], false);
      HCK(hipEventRecord(ctx->join[c], ctx->sub[c]));
      HCK(hipStreamWaitEvent(home, ctx->join[c], 0));
      g0 = g1;
    }
  }
  check_launch(ctx);
}

void verify_one(dkg_ctx* ctx, size_t n, size_t t, int round, size_t D, size_t dealer_base, const uint32_t* Ccomp,
                const uint32_t* s, const uint32_t* sp, uint8_t* dec, bool timed, const uint8_t* extra_ok = nullptr) {
  VerifySeg g{round, D, dealer_base, Ccomp, s, sp, dec, extra_ok};
  verify_device(ctx, n, t, &g, 1, timed, round == 2 ? "r2" : "r4");
}

// Rounds 2 and 4 of one set of dealers.  ctx->overlap (default): one fused pipeline over both
// commitment vectors -- the round-4 inputs (A_i, s_ij) are fixed in round 1 and only the SKIPPED
// mask applied afterwards depends on round 2, so every output is identical to protocol order.
// Otherwise round 2, then (after `between`, e.g. round 3) round 4, each timed when nsub == 1.
// `after2` (may be null) is recorded on ctx->stream once the round-2 decisions are complete.
// e_ok (may be null): per-dealer device mask, 0 = the dealer's round-1 data is missing (round 2:
// DKG_MISSING); a_ok (may be null): 0 = its phase-3 commitments are missing (round 4: accusation)
// (full mode), folded into the round-2 decisions like an undecodable commitment.
// host_between = false (fused rounds only): `between` only queues device work, so it follows the
// checks on the stream without a host round trip; the caller syncs and calls collect_verify_phases.
template <typename F>
void verify_rounds_group(dkg_ctx* ctx, size_t n, size_t t, size_t D, size_t dealer_base, const uint32_t* Ecomp,
                         const uint32_t* Acomp, const uint32_t* s, const uint32_t* sp, uint8_t* dec2, uint8_t* dec4,
                         hipEvent_t after2, F&& between, const uint8_t* e_ok, const uint8_t* a_ok,
                         bool host_between) {
  if (ctx->overlap) {
    VerifySeg g[2] = {{2, D, dealer_base, Ecomp, s, sp, dec2, e_ok}, {4, D, dealer_base, Acomp, s, nullptr, dec4, a_ok}};
    verify_device(ctx, n, t, g, 2, true, "r24");
    if (after2) HCK(hipEventRecord(after2, ctx->stream));
    if (host_between) {
      sync(ctx);
      collect_verify_phases(ctx);
    }
    between();
  } else {
    VerifySeg g2{2, D, dealer_base, Ecomp, s, sp, dec2, e_ok};
    verify_device(ctx, n, t, &g2, 1, true, "r2");
    if (after2) HCK(hipEventRecord(after2, ctx->stream));
    sync(ctx);
    collect_verify_phases(ctx);
    between();
    verify_one(ctx, n, t, 4, D, dealer_base, Acomp, s, nullptr, dec4, true, a_ok);
    sync(ctx);
    collect_verify_phases(ctx);
  }
}

// ---- committee verification by interpolation (ctx->verify_mode == 1; interp.hip) ----
// Inverse Vandermonde of the points 1..N mod l in Montgomery form, [x^k] L_j(x) * 2^256 (L_j the
// Lagrange basis polynomial of point j+1), as 11 limbs of 24 bits: W24[j][a][k] (k_interp).
// Cached per N.
const uint32_t* vinv_table(dkg_ctx* ctx, size_t N) {
  uint32_t* dev = buf<uint32_t>(ctx, "v.vinv", 4 * 11 * N * N);
  if (ctx->vinv_N == N) return dev;
  using dkgh::Zl;
  const Zl zero = dkgh::zl_from_u64(0);
  std::vector<Zl> M(N + 1, zero);  // M(x) = prod_m (x - (m+1)), ascending coefficients
  M[0] = dkgh::zl_from_u64(1);
  for (size_t m = 0; m < N; m++) {
    const Zl xm = dkgh::zl_from_u64(m + 1);
    for (size_t k = m + 1; k > 0; k--) M[k] = dkgh::zl_sub(M[k - 1], dkgh::zl_mul(xm, M[k]));
    M[0] = dkgh::zl_sub(zero, dkgh::zl_mul(xm, M[0]));
  }
  uint8_t r256[33] = {0};
  r256[32] = 1;
  const Zl R = dkgh::zl_from_bytes_wide(r256, 33);  // 2^256 mod l
  std::vector<uint32_t> host(11 * N * N);
  std::vector<Zl> q(N);
  for (size_t j = 0; j < N; j++) {
    const Zl xj = dkgh::zl_from_u64(j + 1);
    q[N - 1] = M[N];  // Q_j = M / (x - x_j), synthetic division
    for (size_t k = N - 1; k > 0; k--) q[k - 1] = dkgh::zl_add(M[k], dkgh::zl_mul(xj, q[k]));
    Zl den = zero;  // Q_j(x_j) = prod_{m != j} (x_j - x_m)
    for (size_t k = N; k-- > 0;) den = dkgh::zl_add(dkgh::zl_mul(den, xj), q[k]);
    const Zl scale = dkgh::zl_mul(dkgh::zl_inv(den), R);
    for (size_t k = 0; k < N; k++) {
      uint8_t b[33] = {0};
      dkgh::zl_to_bytes(b, dkgh::zl_mul(q[k], scale));
      for (size_t a = 0; a < 11; a++) {  // bits 24a .. 24a+23
        const size_t by = 3 * a;
        host[(j * 11 + a) * N + k] = (uint32_t)b[by] | (uint32_t)b[by + 1] << 8 | (uint32_t)b[by + 2] << 16;
      }
    }
  }
  h2d(ctx, dev, host.data(), 4 * host.size());
  ctx->vinv_N = N;
  return dev;
}

enum { IP_INTERPOLATE, IP_COEF_CHECK, IP_DECIDE, IP_FALLBACK };
const PhaseRow INTERP_PHASES[] = {{"interpolate", 1u << IP_INTERPOLATE}, {"coef_check", 1u << IP_COEF_CHECK},
                                  {"decide", 1u << IP_DECIDE}, {"fallback", 1u << IP_FALLBACK}};

template <typename F>
void verify_rounds_interp(dkg_ctx* ctx, size_t n, size_t t, size_t D, size_t dealer_base, const uint32_t* Ecomp,
                          const uint32_t* Acomp, const uint32_t* s, const uint32_t* sp, uint8_t* dec2, uint8_t* dec4,
                          hipEvent_t after2, F&& between, const uint8_t* e_ok, const uint8_t* a_ok) {
  const size_t N = t + 1;
  hipStream_t st = ctx->stream;
  if (D) {
    phase_mark(ctx, st, "interp", -1);
    // the commitments as group elements [D][N]
    const uint32_t *Ee, *Ae;
    size_t cs;
    uint8_t* dokE = buf<uint8_t>(ctx, "i.dokE", D);
    uint8_t* dokA = buf<uint8_t>(ctx, "i.dokA", D);
    if (ctx->ext_E) {
      Ee = ctx->ext_E;
      Ae = ctx->ext_A;
      cs = ctx->ext_stride;
      HCK(hipMemsetAsync(dokE, 1, D, st));
      HCK(hipMemsetAsync(dokA, 1, D, st));
    } else {  // K5 (groups.rs:78-81): a row that does not decode is missing data
      uint32_t* ee = buf<uint32_t>(ctx, "i.Eext", PTB * D * N);
      uint32_t* ae = buf<uint32_t>(ctx, "i.Aext", PTB * D * N);
      uint8_t* pok = buf<uint8_t>(ctx, "i.pok", D * N);
      dkgk::decode_points(Ecomp, D * N, ee, D * N, pok, st);
      dkgk::dealer_ok(D, N, pok, dokE, st);
      dkgk::decode_points(Acomp, D * N, ae, D * N, pok, st);
      dkgk::dealer_ok(D, N, pok, dokA, st);
      Ee = ee;
      Ae = ae;
      cs = D * N;
    }
    dkgk::and_mask(D, e_ok, dokE, st);
    dkgk::and_mask(D, a_ok, dokA, st);
    const uint32_t* WT = vinv_table(ctx, N);
    uint32_t* Fa = buf<uint32_t>(ctx, "i.F", 32 * D * N);
    uint32_t* Fb = buf<uint32_t>(ctx, "i.Fp", 32 * D * N);
    dkgk::interp(D, N, n, WT, s, sp, Fa, Fb, st);  // F, F' through receivers 1..t+1
    phase_mark(ctx, st, "interp", IP_INTERPOLATE);
    uint8_t* okE = buf<uint8_t>(ctx, "i.okE", D * N);
    uint8_t* okA = buf<uint8_t>(ctx, "i.okA", D * N);
    dkgk::coef_check(D, N, Fa, Fb, Ee, Ae, cs, ctx->tab_gw, ctx->tab_hw, okE, okA, st);
    uint8_t* cE = buf<uint8_t>(ctx, "i.cE", D);
    uint8_t* cA = buf<uint8_t>(ctx, "i.cA", D);
    dkgk::dealer_ok(D, N, okE, cE, st);
    dkgk::dealer_ok(D, N, okA, cA, st);
    phase_mark(ctx, st, "interp", IP_COEF_CHECK);
    dkgk::interp_decide(D, n, N, dealer_base, n, s, sp, Fa, Fb, dokE, dokA, cE, cA, ctx->tab_gw, ctx->tab_hw, dec2,
                        dec4, st);
    phase_mark(ctx, st, "interp", IP_DECIDE);
    check_launch(ctx);
    // rows whose commitments are not g F + h F' (case B): difference tables, every P_i(j) in the group
    std::vector<uint8_t> h_dE(D), h_dA(D), h_cE(D), h_cA(D);
    d2h(ctx, h_dE.data(), dokE, D);
    d2h(ctx, h_dA.data(), dokA, D);
    d2h(ctx, h_cE.data(), cE, D);
    d2h(ctx, h_cA.data(), cA, D);
    sync(ctx);
    std::vector<size_t> rows;
    for (size_t d = 0; d < D; d++)
      if ((h_dE[d] && !h_cE[d]) || (h_dA[d] && !h_cA[d])) rows.push_back(d);
    if (!rows.empty()) {
      const size_t R = rows.size();
      uint32_t* rs = buf<uint32_t>(ctx, "i.rs", 32 * R * n);
      uint32_t* rsp = buf<uint32_t>(ctx, "i.rsp", 32 * R * n);
      uint8_t* r2 = buf<uint8_t>(ctx, "i.r2", R * n);
      uint8_t* r4 = buf<uint8_t>(ctx, "i.r4", R * n);
      uint32_t *rE = nullptr, *rA = nullptr, *rEx = nullptr, *rAx = nullptr;
      if (ctx->ext_E) {
        rEx = buf<uint32_t>(ctx, "i.rEx", PTB * R * N);
        rAx = buf<uint32_t>(ctx, "i.rAx", PTB * R * N);
      } else {
        rE = buf<uint32_t>(ctx, "i.rE", 32 * R * N);
        rA = buf<uint32_t>(ctx, "i.rA", 32 * R * N);
      }
      for (size_t r = 0; r < R; r++) {
        const size_t d = rows[r];
        HCK(hipMemcpyAsync(rs + 8 * r * n, s + 8 * d * n, 32 * n, hipMemcpyDeviceToDevice, st));
        HCK(hipMemcpyAsync(rsp + 8 * r * n, sp + 8 * d * n, 32 * n, hipMemcpyDeviceToDevice, st));
        if (rEx) {  // SoA planes: 40 words x N points per row
          HCK(hipMemcpy2DAsync(rEx + r * N, 4 * R * N, ctx->ext_E + d * N, 4 * ctx->ext_stride, 4 * N, PT_WORDS_H,
                               hipMemcpyDeviceToDevice, st));
          HCK(hipMemcpy2DAsync(rAx + r * N, 4 * R * N, ctx->ext_A + d * N, 4 * ctx->ext_stride, 4 * N, PT_WORDS_H,
                               hipMemcpyDeviceToDevice, st));
        } else {
          HCK(hipMemcpyAsync(rE + 8 * r * N, Ecomp + 8 * d * N, 32 * N, hipMemcpyDeviceToDevice, st));
          HCK(hipMemcpyAsync(rA + 8 * r * N, Acomp + 8 * d * N, 32 * N, hipMemcpyDeviceToDevice, st));
        }
      }
      // fused round-2/4 pipeline on the compact rows; dealer_base = n with modulus 2n + R marks no
      // pair as self (the diagonal is restored below)
      const uint32_t *sE = ctx->ext_E, *sA = ctx->ext_A;
      const size_t sstr = ctx->ext_stride;
      if (rEx) {
        ctx->ext_E = rEx;
        ctx->ext_A = rAx;
        ctx->ext_stride = R * N;
      }
      VerifySeg g[2] = {{2, R, n, rE, rs, rsp, r2, nullptr, 2 * n + R}, {4, R, n, rA, rs, nullptr, r4, nullptr, 2 * n + R}};
      const bool ov = ctx->overlap;
      ctx->overlap = true;
      verify_device(ctx, n, t, g, 2, false, "");
      ctx->overlap = ov;
      ctx->ext_E = sE;
      ctx->ext_A = sA;
      ctx->ext_stride = sstr;
      for (size_t r = 0; r < R; r++) {
        const size_t d = rows[r], jself = (d + dealer_base) % n;
        if (h_dE[d] && !h_cE[d]) {
          HCK(hipMemcpyAsync(dec2 + d * n, r2 + r * n, n, hipMemcpyDeviceToDevice, st));
          HCK(hipMemsetAsync(dec2 + d * n + jself, DKG_SELF, 1, st));
        }
        if (h_dA[d] && !h_cA[d]) {
          HCK(hipMemcpyAsync(dec4 + d * n, r4 + r * n, n, hipMemcpyDeviceToDevice, st));
          HCK(hipMemsetAsync(dec4 + d * n + jself, DKG_SELF, 1, st));
        }
      }
      check_launch(ctx);
    }
    phase_mark(ctx, st, "interp", IP_FALLBACK);  // spans the host round trip after the decisions
    ctx->fallback_rows = rows.size();
  }
  if (after2) HCK(hipEventRecord(after2, st));
  sync(ctx);
  if (D) phase_collect(ctx, "interp", INTERP_PHASES, std::size(INTERP_PHASES));
  between();
}

template <typename F>
void verify_rounds(dkg_ctx* ctx, size_t n, size_t t, size_t D, size_t dealer_base, const uint32_t* Ecomp,
                   const uint32_t* Acomp, const uint32_t* s, const uint32_t* sp, uint8_t* dec2, uint8_t* dec4,
                   hipEvent_t after2, F&& between, const uint8_t* e_ok = nullptr, const uint8_t* a_ok = nullptr,
                   bool host_between = true) {
  // dkg_ctx_stepping_redos reports THIS verification's stepping (none if it builds no tables)
  ctx->last_step_flags = nullptr;
  ctx->last_step_flag_words = 0;
  ctx->last_bflags = nullptr;
  ctx->last_bflag_words = 0;
  ctx->binom_any = nullptr;
  ctx->binom_any_host = nullptr;
  if (ctx->binom_step_ded && DKG_BINOM_STEP_DED == 1) {  // both rounds' binomials mark one word
    ctx->binom_any = buf<uint32_t>(ctx, "v.bany", 4);
    HCK(hipMemsetAsync(ctx->binom_any, 0, 4, ctx->stream));
  }
  if (ctx->verify_mode == 1)
    verify_rounds_interp(ctx, n, t, D, dealer_base, Ecomp, Acomp, s, sp, dec2, dec4, after2, between, e_ok, a_ok);
  else
    verify_rounds_group(ctx, n, t, D, dealer_base, Ecomp, Acomp, s, sp, dec2, dec4, after2, between, e_ok, a_ok,
                        host_between);
}

// Queues the copy of the rerun guard's word into pinned memory ahead of the caller's own sync, so
// that reading it costs no round trip of its own.
void binom_mark_copy(dkg_ctx* ctx) {
  if (!ctx->binom_any) return;
  uint32_t* h = hbuf<uint32_t>(ctx, "bany.h", 4);
  d2h(ctx, h, ctx->binom_any, 4);
  ctx->binom_any_host = h;
}

// After a sync: did the last verification's per-step binomial mark a group (a dedicated addition met
// Z = 0)?  Then its tables are not the complete formula's and the caller reruns the verification.
// (A caller that queued no copy pays a blocking read.)
bool binom_marked(dkg_ctx* ctx) {
  if (!ctx->binom_any) return false;
  uint32_t v = 0;
  if (ctx->binom_any_host)
    v = *ctx->binom_any_host;
  else
    HCK(hipMemcpy(&v, ctx->binom_any, 4, hipMemcpyDeviceToHost));
  return v != 0;
}

// Runs f() -- a verification and its outcomes, ending in a sync -- with the per-step binomial's
// dedicated additions allowed; when a group was marked, f() runs again with the complete formula.
template <typename F>
void with_binom_ded(dkg_ctx* ctx, F&& f) {
  struct Off {
    dkg_ctx* c;
    ~Off() { c->binom_step_ded = false; }
  } off{ctx};
  ctx->binom_step_ded = true;
  ctx->last_binom_rerun = 0;
  f();
  ctx->binom_step_ded = false;
  if (binom_marked(ctx)) {
    ctx->last_binom_rerun = 1;
    f();
  }
}

double ev_ms(dkg_ctx* ctx, int a, int b) {
  float ms = 0;
  HCK(hipEventElapsedTime(&ms, ctx->ev[a], ctx->ev[b]));
  return ms;
}

// Lagrange coefficients at zero (polynomial.rs:162-170 with x = 0) over the abscissae x = j + 1 of
// the parties j < n with in_set[j]: lambda_a = prod_{b != a} x_b / (x_b - x_a).  Over the full
// range 1..n the denominator is (-1)^(x_a - 1) (x_a - 1)! (n - x_a)!, so with U = {1..n}
//   lambda_a = P * prod_{e in U \ set} (x_e - x_a) * (-1)^j / ((j+1)! (n-1-j)!),  P = prod_set x_b,
// which costs O(n + |set| * |U \ set|) multiplications and one inversion (inverse factorials),
// instead of |set|^2 products and |set| inversions.  Zero for j outside the set.
std::vector<dkgh::Zl> lagrange_zero_coeffs(size_t n, const uint8_t* in_set) {
  using namespace dkgh;
  const Zl zero = zl_from_u64(0), one = zl_from_u64(1);
  std::vector<Zl> fact(n + 1), ifact(n + 1), lam(n, zero);
  fact[0] = one;
  for (size_t k = 1; k <= n; k++) fact[k] = zl_mul(fact[k - 1], zl_from_u64(k));
  ifact[n] = zl_inv(fact[n]);
  for (size_t k = n; k > 0; k--) ifact[k - 1] = zl_mul(ifact[k], zl_from_u64(k));
  Zl P = one;
  std::vector<size_t> outside;
  for (size_t j = 0; j < n; j++) {
    if (in_set[j]) P = zl_mul(P, zl_from_u64(j + 1));
    else outside.push_back(j);
  }
  for (size_t j = 0; j < n; j++) {
    if (!in_set[j]) continue;
    Zl v = zl_mul(P, zl_mul(ifact[j + 1], ifact[n - 1 - j]));
    for (size_t e : outside) v = zl_mul(v, zl_sub(zl_from_u64(e + 1), zl_from_u64(j + 1)));
    lam[j] = (j & 1) ? zl_sub(zero, v) : v;
  }
  return lam;
}

// sum_j lambda[j] * y[j] with y[j] the 32-byte scalar at ys + 32 * j (j < n, lambda[j] != 0)
dkgh::Zl lagrange_dot(const std::vector<dkgh::Zl>& lam, const uint8_t* ys, size_t n) {
  dkgh::Zl acc = dkgh::zl_from_u64(0);
  for (size_t j = 0; j < n; j++)
    if (!dkgh::zl_is_zero(lam[j])) acc = dkgh::zl_add(acc, dkgh::zl_mul(lam[j], dkgh::zl_from_bits(ys + 32 * j)));
  return acc;
}

// The final parties of finalise: qualified and not reconstructable (committee.rs:733-739).
std::vector<uint8_t> final_parties(size_t n, const uint8_t* qualified, const uint8_t* recon) {
  std::vector<uint8_t> f(n);
  for (size_t j = 0; j < n; j++) f[j] = qualified[j] && !recon[j];
  return f;
}

// The final parties whose phase-5 disclosures reach the others: a party whose Phase1 or Phase3
// proceed failed (r2 / r4 error, committee.rs:340-347, 567-569) never reaches Phases<Phase4>::proceed
// and never broadcasts a BroadcastPhase5 (:684); it does not finalise either.  r2err / r4err may be
// null (no errors).
std::vector<uint8_t> disclosing_parties(size_t n, const uint8_t* qualified, const uint8_t* recon, const uint8_t* r2err,
                                        const uint8_t* r4err) {
  std::vector<uint8_t> f = final_parties(n, qualified, recon);
  for (size_t j = 0; j < n; j++) f[j] = f[j] && !(r2err && r2err[j]) && !(r4err && r4err[j]);
  return f;
}

// With reconstructed dealers, every finalising party holds its own share plus the other disclosing
// final parties' -- exactly the disclosing set S -- and fails with InsufficientSharesForRecovery when
// that is fewer than `threshold` = t points (:779-781): then no party has an mpk.
bool recovery_fails(const std::vector<uint8_t>& S, size_t t) {
  size_t c = 0;
  for (auto v : S) c += v != 0;
  return c < t;
}

// Secrets of the reconstructed dealers (rows `rows` of hs, share row r at hs + 32 * n * r) as the
// finalising parties recover them: a final party p interpolates dealer i's shares at its own index
// and at every other disclosing final party's (committee.rs:754-788), i.e. at exactly the disclosing
// set `fin` (disclosing_parties), so every finalising party computes this same value (with exactly t
// points a wrong one, as the reference does; the per-party view with missing disclosures is
// dkg_finalise_parties).  The dealer's share to itself is never used (it is not a final party), and
// its other shares all passed round 2.
std::vector<uint8_t> recon_secrets(size_t n, const std::vector<uint8_t>& fin, const uint8_t* hs,
                                   const std::vector<size_t>& rows) {
  const std::vector<dkgh::Zl> lam = lagrange_zero_coeffs(n, fin.data());
  std::vector<uint8_t> secrets(32 * rows.size());
  for (size_t r = 0; r < rows.size(); r++) dkgh::zl_to_bytes(&secrets[32 * r], lagrange_dot(lam, hs + 32 * n * rows[r], n));
  return secrets;
}

// Round-2 outcome of `groups` stacked ceremonies of n parties from the decision matrix
// dec2 [groups*n][n] on the device, as every party derives it (committee.rs:311-347, 370-398): a
// REJECT by receiver j is a complaint of j against dealer i, and a valid complaint disqualifies i for
// everyone; MISSING (no decodable broadcast) disqualifies without a complaint (:331-335); more than t
// complaints raise MisbehaviourHigherThreshold for j (:340-347); qmask (device [groups*n]) receives
// the qualified set.  Each round's outcome has a device half (kernels queued on ctx->stream, the
// per-dealer / per-receiver results left in `rej`, `cnt`, `r4d`) and a host half (applied to their
// copies after a sync), so that a caller queues both rounds' device halves and copies everything back
// in one round trip.  The single-GPU drivers, the batches and the sharded combine all decide through
// these four functions.
// cmask (device [groups*n], may be null): the qualified set by PROVEN complaints instead -- cmask[i] = no
// verified complaint against i (compute_qualified_set, :370-398, run on the broadcast complaints by
// the caller): a row is then disqualified by MISSING or by cmask only, a REJECT alone keeps it.
void round2_device(dkg_ctx* ctx, size_t groups, size_t n, const uint8_t* dec2, uint8_t* qmask, uint8_t* rej,
                   int32_t* cnt, const uint8_t* cmask = nullptr) {
  dkgk::decision_summary(groups, n, dec2, rej, cnt, ctx->stream);
  if (cmask) dkgk::qualified_complaints(groups * n, n, dec2, cmask, rej, qmask, ctx->stream);
  else dkgk::mask_not_and(groups * n, rej, nullptr, qmask, ctx->stream);  // qualified = no rejecting row
}
// host half: `qualified` holds the copied rej flags on entry
void round2_host(size_t V, size_t t, uint8_t* qualified, const int32_t* complaints, uint8_t* r2err) {
  for (size_t i = 0; i < V; i++) {
    qualified[i] = !qualified[i];
    r2err[i] = complaints[i] > (int32_t)t;  // committee.rs:340-347
  }
}
// Round-4 outcome (committee.rs:515-522, 567-569, 660-670) from dec4 [groups*n][n] on the device and
// the round-2 qualified set (host `qualified`, device `qmask`): the rows of disqualified dealers
// become SKIPPED in place (:522); a qualified dealer some receiver rejects is reconstructed; receiver
// j's round-4 error (r4d / r4err, may be NULL) counts itself and the qualified dealers it accepted.
void round4_device(dkg_ctx* ctx, size_t groups, size_t n, size_t t, uint8_t* dec4, const uint8_t* qmask,
                   uint8_t* rej, uint8_t* r4d) {
  dkgk::decision_summary(groups, n, dec4, rej, nullptr, ctx->stream);
  if (r4d) dkgk::r4_error(groups, n, t, dec4, qmask, r4d, ctx->stream);
  dkgk::apply_skipped(groups, n, dec4, qmask, ctx->stream);
}
// host half: `recon` holds the copied rej flags on entry
void round4_host(size_t V, const uint8_t* qualified, uint8_t* recon) {
  for (size_t i = 0; i < V; i++) recon[i] = qualified[i] && recon[i];
}

// Rounds 2-5 on device-resident broadcast values (E, A compressed [n][N][8]; s, sp [n][n][8]).
// The outcomes stay on the device until the end -- one host round trip per ceremony, as the batches
// (batch_receivers): the round-2 outcome's device half gives the qualified mask for round 3, the
// round-4 half the reconstruction flags, and the master key is summed over the honest set (qualified,
// not reconstructed: committee.rs:726-805) speculatively; the host then only zeroes it (Phase4 failure,
// failed recovery) or, when a dealer is reconstructed, adds g * its recovered secret (a second trip).
// Per-dealer masks on the device ([n], null = absent).  e_ok / a_ok: the e_ok / a_ok of verify_rounds
// (an intake mask, or the decode mask of the dealer's ciphertexts).  cmask: the qualified set follows
// the PROVEN round-2 complaints (round2_device) instead of the receivers' own rejections.  proven4: the
// reconstructable set follows the PROVEN round-4 complaints -- proven4[i] = some broadcast complaint
// against i holds (Phases<Phase4>::proceed, committee.rs:636-670, run on the complaints by the
// caller); a receiver's own rejection alone reconstructs nobody.
struct RoundMasks {
  const uint8_t *e_ok = nullptr, *a_ok = nullptr, *cmask = nullptr, *proven4 = nullptr;
};
// The parties' common outcome, as written to dkg_ceremony_out where the caller gave arrays.
struct RoundsResult {
  std::vector<uint8_t> qualified, reconstruct, r2_error, r4_error;
  int32_t n_qualified = 0;
  bool phase4_error = false;
};
RoundsResult receivers_rounds_once(dkg_ctx* ctx, size_t n, size_t t, const uint32_t* Ecomp, const uint32_t* Acomp,
                                   const uint32_t* s, const uint32_t* sp, dkg_ceremony_out* out, bool copy_big,
                                   const RoundMasks& m) {
  const size_t N = t + 1;
  uint8_t* dec2 = buf<uint8_t>(ctx, "dec2", n * n);
  uint8_t* dec4 = buf<uint8_t>(ctx, "dec4", n * n);
  uint32_t* fs = buf<uint32_t>(ctx, "final_share", 32 * n);
  uint32_t* pubc = buf<uint32_t>(ctx, "pub_comp", 32 * n);
  uint8_t* qmask = buf<uint8_t>(ctx, "qmask", n);
  uint8_t* rej2 = buf<uint8_t>(ctx, "o.rej2", n);
  int32_t* cnt = buf<int32_t>(ctx, "o.cnt", 4 * n);
  // ---- rounds 2 and 4 (committee.rs:260-366, :508-580), fused or in protocol order (verify_rounds)
  auto round3 = [&] {
    wait_shares(ctx, ctx->stream);
    round2_device(ctx, 1, n, dec2, qmask, rej2, cnt, m.cmask);
    // ---- round 3 (committee.rs:433-476): final share s_j = sum_{i in Q} s_ij, public g s_j
    dkgk::sum_shares(n, n, s, qmask, fs, ctx->stream);
    // the public shares g s_j are an output only: computed on the side stream, off the path to
    // round 4 and finalise (joined before the outputs are read)
    uint32_t* pub = buf<uint32_t>(ctx, "pub_ext", PTB * n);
    HCK(hipEventRecord(ctx->side_fork, ctx->stream));
    HCK(hipStreamWaitEvent(ctx->side, ctx->side_fork, 0));
    dkgk::fixed_base(n, fs, ctx->tab_gw, pub, ctx->side);
    dkgk::encode_points(pub, n, n, pubc, ctx->side);
    HCK(hipEventRecord(ctx->pub_done, ctx->side));
    HCK(hipEventRecord(ctx->ev[3], ctx->stream));
  };
  verify_rounds(ctx, n, t, n, 0, Ecomp, Acomp, s, sp, dec2, dec4, ctx->ev[2], round3, m.e_ok, m.a_ok, false);
  wait_shares(ctx, ctx->stream);
  ctx->shares_pending = false;
  // round-4 outcome on the device: a qualified dealer some receiver rejects is reconstructed
  // (committee.rs:660-670); receiver j's round-4 error (:515-516, 567-569) counts itself and the
  // qualified dealers it accepted
  uint8_t* rej4 = buf<uint8_t>(ctx, "o.rej4", n);
  uint8_t* r4d = buf<uint8_t>(ctx, "o.r4err", n);
  round4_device(ctx, 1, n, t, dec4, qmask, rej4, r4d);
  // the proven complaints' mask stands in for the rejections; the qualified mask is applied below
  // to either (:639)
  const uint8_t* acc4 = m.proven4 ? m.proven4 : rej4;
  HCK(hipEventRecord(ctx->ev[4], ctx->stream));
  // ---- finalise (committee.rs:726-805): mpk = sum_{i in Q \ recon} A_i0 (+ sum_{recon} g * L_i(0))
  uint32_t* A0 = buf<uint32_t>(ctx, "A0ext", PTB * n);
  if (ctx->ext_A) {
    dkgk::gather_points(ctx->ext_A, ctx->ext_stride, N, 0, n, A0, n, ctx->stream);
  } else {
    uint32_t* A0c = buf<uint32_t>(ctx, "A0c", 32 * n);
    HCK(hipMemcpy2DAsync(A0c, 32, Acomp, 32 * N, 32, n, hipMemcpyDeviceToDevice, ctx->stream));
    uint8_t* a0ok = buf<uint8_t>(ctx, "A0ok", n);
    dkgk::decode_points(A0c, n, A0, n, a0ok, ctx->stream);
  }
  uint8_t* hmask = buf<uint8_t>(ctx, "hmask", n);
  dkgk::mask_not_and(n, acc4, qmask, hmask, ctx->stream);  // the final parties: qualified, not accused
  uint32_t* mpk_ext = buf<uint32_t>(ctx, "mpk_ext", PTB);
  dkgk::sum_points(n, A0, n, hmask, mpk_ext, 1, 0, ctx->stream);
  uint32_t* mpk_c = buf<uint32_t>(ctx, "mpk_comp", 32);
  dkgk::encode_points(mpk_ext, 1, 1, mpk_c, ctx->stream);
  check_launch(ctx);
  uint8_t* h = hbuf<uint8_t>(ctx, "rr.out", 8 * n + 32);  // rej2 | rej4 | r4err | cnt | mpk
  d2h(ctx, h, rej2, n);
  d2h(ctx, h + n, acc4, n);
  d2h(ctx, h + 2 * n, r4d, n);
  d2h(ctx, h + 3 * n, cnt, 4 * n);
  d2h(ctx, h + 7 * n, mpk_c, 32);
  HCK(hipEventRecord(ctx->ev[5], ctx->stream));
  HCK(hipStreamWaitEvent(ctx->stream, ctx->pub_done, 0));  // public shares (round 3, side stream)
  if (copy_big) {
    if (out->dec2) d2h(ctx, out->dec2, dec2, n * n);
    if (out->dec4) d2h(ctx, out->dec4, dec4, n * n);  // SKIPPED rows applied (round4_device)
    if (out->final_share) d2h(ctx, out->final_share, fs, 32 * n);
    if (out->public_share) d2h(ctx, out->public_share, pubc, 32 * n);
  }
  binom_mark_copy(ctx);
  sync(ctx);
  collect_verify_phases(ctx);
  std::vector<uint8_t> qualified(h, h + n), r2err(n), recon(h + n, h + 2 * n), r4e(h + 2 * n, h + 3 * n);
  std::vector<int32_t> complaints(n);
  memcpy(complaints.data(), h + 3 * n, 4 * n);
  round2_host(n, t, qualified.data(), complaints.data(), r2err.data());
  round4_host(n, qualified.data(), recon.data());
  const std::vector<uint8_t> disc = disclosing_parties(n, qualified.data(), recon.data(), r2err.data(), r4e.data());
  size_t nrecon = 0;
  int32_t nq = 0;
  for (size_t i = 0; i < n; i++) {
    nrecon += recon[i];
    nq += qualified[i];
  }
  // Phases<Phase4>::proceed fails for every party when qualified minus reconstructable <= t
  // (committee.rs:673-677): nobody finalises, so there is no master public key (mpk zeroed); with
  // reconstructions and fewer than t disclosing parties nobody recovers (:779-781): none either
  const bool phase4_error = nq - (int32_t)nrecon <= (int32_t)t;
  memset(out->mpk, 0, 32);
  if (!phase4_error && !(nrecon && recovery_fails(disc, t))) {
    if (nrecon) {  // + g * the reconstructed secrets, interpolated over the disclosing final parties
      std::vector<size_t> rows;
      std::vector<uint8_t> hs(32 * n * nrecon);
      for (size_t i = 0; i < n; i++)
        if (recon[i]) {
          d2h(ctx, &hs[32 * n * rows.size()], s + 8 * n * i, 32 * n);
          rows.push_back(rows.size());
        }
      sync(ctx);
      std::vector<uint8_t> secrets = recon_secrets(n, disc, hs.data(), rows);
      uint32_t* sec = buf<uint32_t>(ctx, "recon_sec", 32 * nrecon);
      h2d(ctx, sec, secrets.data(), secrets.size());
      uint32_t* gsec = buf<uint32_t>(ctx, "recon_ext", PTB * nrecon);
      uint32_t* extra = buf<uint32_t>(ctx, "recon_sum", PTB);
      dkgk::fixed_base(nrecon, sec, ctx->tab_gw, gsec, ctx->stream);
      dkgk::sum_points(nrecon, gsec, nrecon, nullptr, extra, 1, 0, ctx->stream);
      dkgk::add_points(1, mpk_ext, extra, 1, mpk_ext, ctx->stream);
      dkgk::encode_points(mpk_ext, 1, 1, mpk_c, ctx->stream);
      check_launch(ctx);
      d2h(ctx, h + 7 * n, mpk_c, 32);
      sync(ctx);
    }
    memcpy(out->mpk, h + 7 * n, 32);
  }
  // ---- outputs
  if (out->qualified) memcpy(out->qualified, qualified.data(), n);
  if (out->r2_error) memcpy(out->r2_error, r2err.data(), n);
  if (out->r4_error) memcpy(out->r4_error, r4e.data(), n);
  if (out->complaints2) memcpy(out->complaints2, complaints.data(), 4 * n);
  if (out->reconstruct) memcpy(out->reconstruct, recon.data(), n);
  out->n_qualified = nq;
  out->phase4_error = phase4_error;  // committee.rs:673-677
  return {std::move(qualified), std::move(recon), std::move(r2err), std::move(r4e), nq, phase4_error};
}

// receivers_rounds_once with the per-step binomial's dedicated additions, rerun with the complete
// formula when they marked a group (with_binom_ded)
RoundsResult receivers_rounds(dkg_ctx* ctx, size_t n, size_t t, const uint32_t* Ecomp, const uint32_t* Acomp,
                              const uint32_t* s, const uint32_t* sp, dkg_ceremony_out* out, bool copy_big,
                              const RoundMasks& m = {}) {
  RoundsResult r;
  with_binom_ded(ctx, [&] { r = receivers_rounds_once(ctx, n, t, Ecomp, Acomp, s, sp, out, copy_big, m); });
  return r;
}

// The commitments of one ceremony on the device, one array [2n][N][8]: the E rows, then the A rows
// (E is also the whole array, as complaints3_core reads it).
struct Commitments {
  uint32_t *E, *A;
};
Commitments commitment_rows(dkg_ctx* ctx, size_t n, size_t N) {
  uint32_t* EA = buf<uint32_t>(ctx, "cer_EA", 32 * 2 * n * N);
  return {EA, EA + 8 * n * N};
}
Commitments upload_commitments(dkg_ctx* ctx, size_t n, size_t N, const uint8_t* E, const uint8_t* A) {
  const Commitments c = commitment_rows(ctx, n, N);
  h2d(ctx, c.E, E, 32 * n * N);
  h2d(ctx, c.A, A, 32 * n * N);
  return c;
}

void ceremony_times(dkg_ctx* ctx, dkg_ceremony_out* out, bool round1) {
  out->ms_round1 = round1 ? ev_ms(ctx, 0, 1) : 0.0;
  out->ms_round2 = ev_ms(ctx, 1, 2);
  out->ms_round3 = ev_ms(ctx, 2, 3);
  out->ms_round4 = ev_ms(ctx, 3, 4);
  out->ms_finalise = ev_ms(ctx, 4, 5);
  out->ms_total = ev_ms(ctx, 0, 5);
}

// Round 1 for D dealers on device: a, b canonical [D][N][8] -> Ecomp, Acomp [D][N][8], s, sp [D][n][8].
// Round 1 on device.  encode = false: the commitments stay group elements (Ecomp / Acomp are not
// written; the caller verifies through an ExtScope, as the reference's in-memory broadcasts).
// overlap_shares: the share evaluation runs on ctx->side (lowest priority) beside what follows on
// ctx->stream -- the verification's first binomial steps, which occupy few CUs -- and the
// verification's checks and round 3 wait for it (ctx->shares_pending, wait_shares).
void round1_device(dkg_ctx* ctx, size_t D, size_t n, size_t t, const uint32_t* a, const uint32_t* b,
                   uint32_t* Ecomp, uint32_t* Acomp, uint32_t* s, uint32_t* sp, bool encode = true,
                   bool overlap_shares = false) {
  const size_t N = t + 1;
  uint32_t* Aext = buf<uint32_t>(ctx, "Aext", PTB * D * N);
  uint32_t* Eext = buf<uint32_t>(ctx, "Eext", PTB * D * N);
  if (overlap_shares) {  // the side stream starts where ctx->stream is (a, b written)
    HCK(hipEventRecord(ctx->side_fork, ctx->stream));
    HCK(hipStreamWaitEvent(ctx->side, ctx->side_fork, 0));
  }
  dkgk::commit(D * N, a, b, ctx->tab_gw, ctx->tab_hw, Aext, Eext, ctx->stream);  // K2 (committee.rs:151-159)
  if (encode) {
    dkgk::encode_points(Eext, D * N, D * N, Ecomp, ctx->stream);                  // broadcast encodings
    dkgk::encode_points(Aext, D * N, D * N, Acomp, ctx->stream);
  }
  if (overlap_shares) {
    dkgk::share_eval(D, n, N, a, b, s, sp, ctx->side);                             // K1 (:164-167)
    HCK(hipEventRecord(ctx->shares_done, ctx->side));
    ctx->shares_pending = true;
  } else {
    dkgk::share_eval(D, n, N, a, b, s, sp, ctx->stream);
  }
  check_launch(ctx);
}


// Shares evaluated on the side stream (round1_device with overlap_shares) that a call leaves pending
// when it throws: the home stream -- every later call's -- waits for them, then the flag is dropped.
struct SharesScope {
  dkg_ctx* ctx;
  explicit SharesScope(dkg_ctx* c) : ctx(c) {}
  ~SharesScope() {
    if (ctx->shares_pending) (void)hipStreamWaitEvent(ctx->stream, ctx->shares_done, 0);
    ctx->shares_pending = false;
  }
};

// Verify what round1_device just generated from its extended-form commitments (no encode/decode
// round trip); restores the ctx on exit.
struct ExtScope {
  dkg_ctx* ctx;
  ExtScope(dkg_ctx* c, size_t D, size_t N) : ctx(c) {
    ctx->ext_E = buf<uint32_t>(ctx, "Eext", PTB * D * N);
    ctx->ext_A = buf<uint32_t>(ctx, "Aext", PTB * D * N);
    ctx->ext_stride = D * N;
  }
  ~ExtScope() {
    ctx->ext_E = ctx->ext_A = nullptr;
    ctx->ext_stride = 0;
  }
};

// Round 1 of a batch with the commitments deferred into the verification's chunks (r1_a above):
// the fused group pass (verify_mode 0, rounds 2 and 4 fused) computes each chunk's dealers'
// commitments on the chunk's own stream, so the second chunk's commitments (half of config 5's
// round 1) run beside the first chunk's binomial and stepping; the shares are evaluated on the
// side stream beside both.  Other schedules get the whole round 1 first (round1_device).
struct BatchRound1 {
  dkg_ctx* ctx;
  BatchRound1(dkg_ctx* c, size_t D, size_t n, size_t t, const uint32_t* a, const uint32_t* b, uint32_t* s,
              uint32_t* sp)
      : ctx(c) {
    const size_t N = t + 1;
    if (deferred()) {
      HCK(hipEventRecord(ctx->side_fork, ctx->stream));
      HCK(hipStreamWaitEvent(ctx->side, ctx->side_fork, 0));
      dkgk::share_eval(D, n, N, a, b, s, sp, ctx->side);  // K1 (committee.rs:164-167)
      HCK(hipEventRecord(ctx->shares_done, ctx->side));
      ctx->shares_pending = true;
      ctx->r1_a = a;
      ctx->r1_b = b;
      ctx->r1_D = D;
      ctx->r1_A0 = buf<uint32_t>(ctx, "r1_A0", PTB * D);
    } else {
      round1_device(ctx, D, n, t, a, b, nullptr, nullptr, s, sp, false);
    }
    check_launch(ctx);
  }
  bool deferred() const { return ctx->overlap && ctx->verify_mode == 0; }
  ~BatchRound1() {
    // after an exception the shares kernel may still be writing s / sp on the side stream: make the
    // home stream (every later call's) wait for it before the state that tracks it is dropped
    if (ctx->shares_pending) (void)hipStreamWaitEvent(ctx->stream, ctx->shares_done, 0);
    ctx->r1_a = ctx->r1_b = nullptr;
    ctx->r1_D = 0;
    ctx->r1_A0 = nullptr;
    ctx->shares_pending = false;
  }
};

// ---- batches of independent ceremonies (BASELINE config 5: many small key ceremonies)
// B ceremonies of n parties are stacked dealer-wise: dealer c*n + i is party i of ceremony c, and
// its share row addresses that ceremony's n receivers.  The verification pipeline is the same as
// for one ceremony (2*B*n virtual dealers in the fused pipeline); the per-ceremony combine steps
// (qualification, complaints, round-3 sums, mpk) are grouped kernels.  Every output equals what B
// separate ceremonies produce.
// BatchProven (may be null): the batch decides by the PROVEN complaints, as receivers_rounds with
// RoundMasks -- the device masks its complaint stage left (batch_complaints), the host arrays that
// receive the stage's outputs in the batch's one round trip, and the host outcome vectors that
// batch_proven_outcome reads afterwards.
struct BatchProven {
  // device, [V] unless noted; null = absent
  const uint8_t* a_ok = nullptr;     // the intake mask of the phase-3 broadcasts (verify_rounds' a_ok)
  const uint8_t* cmask = nullptr;    // no verified round-2 complaint against the dealer (round2_device)
  const uint8_t* pair = nullptr;     // [V][n] proven (accused, accuser) pairs, for the dissent
  const uint8_t* proven4 = nullptr;  // some round-4 complaint against the dealer holds
  const int32_t *dver2 = nullptr, *dver4 = nullptr;  // the verdicts [C2], [C4]
  size_t C2 = 0, C4 = 0;
  // host outputs (may be null)
  int32_t *verdict2 = nullptr, *verdict4 = nullptr, *dissent = nullptr;
  // host outcome, filled by batch_receivers: a_present[i] = dealer i has a usable phase-3 broadcast
  std::vector<uint8_t> qualified, reconstruct, r2_error, r4_error, phase4_error, a_present;
};
void batch_receivers(dkg_ctx* ctx, size_t B, size_t n, size_t t, const uint32_t* Ecomp, const uint32_t* Acomp,
                     const uint32_t* s, const uint32_t* sp, dkg_batch_out* out, const uint8_t* e_ok = nullptr,
                     BatchProven* bp = nullptr) {
  const size_t N = t + 1, V = B * n;
  uint8_t* dec2 = buf<uint8_t>(ctx, "b.dec2", V * n);
  uint8_t* dec4 = buf<uint8_t>(ctx, "b.dec4", V * n);
  uint8_t* qmask = buf<uint8_t>(ctx, "b.qmask", V);
  uint8_t* rej2 = buf<uint8_t>(ctx, "b.rej2", V);
  uint8_t* rej4 = buf<uint8_t>(ctx, "b.rej4", V);
  uint8_t* r4d = buf<uint8_t>(ctx, "b.r4err", V);
  uint8_t* hmask = buf<uint8_t>(ctx, "b.hmask", V);
  int32_t* cnt = buf<int32_t>(ctx, "b.cnt", 4 * V);
  uint32_t* fs = buf<uint32_t>(ctx, "b.final", 32 * V);
  uint32_t* pub = buf<uint32_t>(ctx, "b.pub_ext", PTB * V);
  uint32_t* pubc = buf<uint32_t>(ctx, "b.pub_comp", 32 * V);
  std::vector<uint8_t> qualified(V), r2err(V), recon(V, 0), honest(V), r4e(V), h_rej4(V);
  std::vector<int32_t> complaints(V);
  // The outcomes stay on the device until the end (one host round trip per batch): the rows that
  // reject or miss disqualify (committee.rs:311-316, 331-335, 370-398), round 3 sums the qualified
  // dealers' shares (:433-476), round 4's rejections reconstruct qualified dealers (:660-670) and the
  // honest set -- qualified, not reconstructed -- sums the master key (:726-805).
  auto round3 = [&] {
    round2_device(ctx, B, n, dec2, qmask, rej2, cnt, bp ? bp->cmask : nullptr);
    wait_shares(ctx, ctx->stream);  // shares evaluated on the side stream (BatchRound1)
    dkgk::sum_shares(n, n, s, qmask, fs, ctx->stream, B);
    dkgk::fixed_base(V, fs, ctx->tab_gw, pub, ctx->stream);
    dkgk::encode_points(pub, V, V, pubc, ctx->stream);
    HCK(hipEventRecord(ctx->ev[3], ctx->stream));
  };
  // e_ok (may be null; [V] on the device): full mode's decode mask of each dealer's ciphertexts -- a row
  // that did not decode is missing data (DKG_MISSING in round 2), as in receivers_rounds
  verify_rounds(ctx, n, t, V, 0, Ecomp, Acomp, s, sp, dec2, dec4, ctx->ev[2], round3, e_ok, bp ? bp->a_ok : nullptr,
                false);
  // round 4 (committee.rs:515-522, 567-569, 660-670): rows of disqualified dealers SKIPPED
  round4_device(ctx, B, n, t, dec4, qmask, rej4, r4d);
  // the proven complaints' mask stands in for the rejections, as in receivers_rounds (:636-670)
  const uint8_t* acc4 = bp && bp->proven4 ? bp->proven4 : rej4;
  dkgk::mask_not_and(V, acc4, qmask, hmask, ctx->stream);
  // by proven complaints the host outcome also needs, per dealer, whether its phase-3 broadcast is
  // usable (present and decodable: proven_outcome's a_ok): the verification's own flags of the A
  // columns, which carry the intake mask -- no second decode of the V N commitments
  uint8_t* apres = nullptr;
  int32_t* ddis = nullptr;
  if (bp) {
    apres = buf<uint8_t>(ctx, "b.apres", V);
    if (ctx->verify_mode == 1) dkgk::segment_mask(V, 1, 0, buf<uint8_t>(ctx, "i.dokA", V), apres, ctx->stream);
    else dkgk::segment_mask(V, ctx->last_dok_nseg, ctx->last_dok_nseg - 1, ctx->last_dok, apres, ctx->stream);
    if (bp->dissent) {  // from the device's dec2 and the proven pairs: dec2 is not downloaded for it
      ddis = buf<int32_t>(ctx, "b.dissent", 4 * V);
      dkgk::dissent_rows(V, n, dec2, bp->pair, ddis, ctx->stream);
    }
  }
  HCK(hipEventRecord(ctx->ev[4], ctx->stream));
  // finalise (committee.rs:726-805): mpk_c = sum of the honest A_i0 (+ g * reconstructed secrets)
  uint32_t* A0 = buf<uint32_t>(ctx, "b.A0ext", PTB * V);
  if (ctx->r1_A0) {  // written by the deferred commitments (k_commit_pm), [40][V]
    HCK(hipMemcpyAsync(A0, ctx->r1_A0, PTB * V, hipMemcpyDeviceToDevice, ctx->stream));
  } else if (ctx->ext_A) {
    dkgk::gather_points(ctx->ext_A, ctx->ext_stride, N, 0, V, A0, V, ctx->stream);
  } else {
    uint32_t* A0c = buf<uint32_t>(ctx, "b.A0c", 32 * V);
    HCK(hipMemcpy2DAsync(A0c, 32, Acomp, 32 * N, 32, V, hipMemcpyDeviceToDevice, ctx->stream));
    uint8_t* a0ok = buf<uint8_t>(ctx, "b.A0ok", V);
    dkgk::decode_points(A0c, V, A0, V, a0ok, ctx->stream);
  }
  uint32_t* mpk_ext = buf<uint32_t>(ctx, "b.mpk_ext", PTB * B);
  dkgk::sum_points(n, A0, V, hmask, mpk_ext, B, 0, ctx->stream, B);
  uint32_t* mpk_c = buf<uint32_t>(ctx, "b.mpk_comp", 32 * B);
  dkgk::encode_points(mpk_ext, B, B, mpk_c, ctx->stream);
  check_launch(ctx);
  // every outcome through pinned staging, one sync: copies into the caller's pageable buffers were
  // staged by the runtime on this thread, 1-27 ms of host time per 10,000-ceremony batch beyond the
  // device span (tools/batch_gap.py)
  struct Out {
    void* host;
    const void* dev;
    size_t bytes;
    const char* name;
  };
  if (bp) bp->a_present.resize(V);
  const Out outs[] = {{qualified.data(), rej2, V, "hb.rej2"},  // inverted below
                      {complaints.data(), cnt, 4 * V, "hb.cnt"},
                      {h_rej4.data(), acc4, V, "hb.rej4"},
                      {r4e.data(), r4d, V, "hb.r4err"},
                      {out->mpk, mpk_c, 32 * B, "hb.mpk"},
                      {out->final_share, fs, 32 * V, "hb.final"},
                      {out->public_share, pubc, 32 * V, "hb.pub"},
                      {out->dec2, dec2, V * n, "hb.dec2"},
                      {out->dec4, dec4, V * n, "hb.dec4"},  // SKIPPED rows applied
                      // by proven complaints: the complaint stage's outputs share the round trip
                      {bp ? bp->a_present.data() : nullptr, apres, V, "hb.apres"},
                      {bp ? bp->verdict2 : nullptr, bp ? bp->dver2 : nullptr, bp ? 4 * bp->C2 : 0, "hb.ver2"},
                      {bp ? bp->verdict4 : nullptr, bp ? bp->dver4 : nullptr, bp ? 4 * bp->C4 : 0, "hb.ver4"},
                      {ddis ? bp->dissent : nullptr, ddis, 4 * V, "hb.dissent"}};
  void* staged[sizeof(outs) / sizeof(outs[0])] = {};
  for (size_t k = 0; k < sizeof(outs) / sizeof(outs[0]); k++)
    if (outs[k].host && outs[k].bytes) {
      staged[k] = hbuf(ctx, outs[k].name, outs[k].bytes);
      d2h(ctx, staged[k], outs[k].dev, outs[k].bytes);
    }
  HCK(hipEventRecord(ctx->ev[5], ctx->stream));
  sync(ctx);
  for (size_t k = 0; k < sizeof(outs) / sizeof(outs[0]); k++)
    if (staged[k]) memcpy(outs[k].host, staged[k], outs[k].bytes);
  collect_verify_phases(ctx);
  round2_host(V, t, qualified.data(), complaints.data(), r2err.data());
  recon = h_rej4;
  round4_host(V, qualified.data(), recon.data());
  for (size_t i = 0; i < V; i++) honest[i] = qualified[i] && !recon[i];
  std::vector<size_t> recon_cer, nompk;
  std::vector<uint8_t> p4err(B, 0);
  for (size_t c = 0; c < B; c++) {
    bool any = false;
    int32_t h = 0;
    for (size_t i = c * n; i < (c + 1) * n; i++) {
      any |= recon[i] != 0;
      h += honest[i];
    }
    p4err[c] = h <= (int32_t)t;  // committee.rs:673-677: nobody finalises, no mpk
    if (any && !p4err[c]) {
      // InsufficientSharesForRecovery for every finalising party: no mpk either (recovery_fails)
      if (recovery_fails(disclosing_parties(n, &qualified[c * n], &recon[c * n], &r2err[c * n], &r4e[c * n]), t))
        nompk.push_back(c);
      else
        recon_cer.push_back(c);
    }
  }
  if (!recon_cer.empty()) {  // ceremonies with round-4 accusations: + g * the reconstructed secrets
    uint32_t* extra = buf<uint32_t>(ctx, "b.mpk_extra", PTB * B);
    std::vector<uint8_t> hs(32 * n * n);
    for (size_t c : recon_cer) {
      d2h(ctx, hs.data(), s + c * n * n * 8, 32 * n * n);
      sync(ctx);
      std::vector<size_t> rows;
      for (size_t i = 0; i < n; i++)
        if (recon[c * n + i]) rows.push_back(i);
      std::vector<uint8_t> secrets = recon_secrets(
          n, disclosing_parties(n, &qualified[c * n], &recon[c * n], &r2err[c * n], &r4e[c * n]), hs.data(), rows);
      const size_t nr = secrets.size() / 32;
      uint32_t* sec = buf<uint32_t>(ctx, "b.recon_sec", 32 * nr);
      h2d(ctx, sec, secrets.data(), secrets.size());
      uint32_t* gsec = buf<uint32_t>(ctx, "b.recon_ext", PTB * nr);
      dkgk::fixed_base(nr, sec, ctx->tab_gw, gsec, ctx->stream);
      dkgk::sum_points(nr, gsec, nr, nullptr, extra, B, c, ctx->stream);
      dkgk::add_points(1, mpk_ext + c, extra + c, B, mpk_ext + c, ctx->stream);
      sync(ctx);  // sec / gsec are reused by the next ceremony
    }
    dkgk::encode_points(mpk_ext, B, B, mpk_c, ctx->stream);
    check_launch(ctx);
    if (out->mpk) d2h(ctx, out->mpk, mpk_c, 32 * B);
    sync(ctx);
  }
  if (out->r4_error) memcpy(out->r4_error, r4e.data(), V);
  if (out->qualified) memcpy(out->qualified, qualified.data(), V);
  if (out->r2_error) memcpy(out->r2_error, r2err.data(), V);
  if (out->complaints2) memcpy(out->complaints2, complaints.data(), 4 * V);
  if (out->reconstruct) memcpy(out->reconstruct, recon.data(), V);
  if (out->phase4_error) memcpy(out->phase4_error, p4err.data(), B);  // committee.rs:673-677
  if (out->mpk) {
    for (size_t c = 0; c < B; c++)
      if (p4err[c]) memset(out->mpk + 32 * c, 0, 32);  // no party finalises: no master key
    for (size_t c : nompk) memset(out->mpk + 32 * c, 0, 32);  // no party recovers the secrets
  }
  if (out->n_qualified)
    for (size_t c = 0; c < B; c++) {
      int32_t q = 0;
      for (size_t i = c * n; i < (c + 1) * n; i++) q += qualified[i];
      out->n_qualified[c] = q;
    }
  if (bp) {
    bp->qualified = std::move(qualified);
    bp->reconstruct = std::move(recon);
    bp->r2_error = std::move(r2err);
    bp->r4_error = std::move(r4e);
    bp->phase4_error = std::move(p4err);
  }
}

void batch_times(dkg_ctx* ctx, dkg_batch_out* out, bool round1) {
  out->ms_round1 = round1 ? ev_ms(ctx, 0, 1) : 0.0;
  out->ms_checks = ev_ms(ctx, 1, 2);
  out->ms_round3 = ev_ms(ctx, 2, 3);
  out->ms_finalise = ev_ms(ctx, 3, 5);
  out->ms_total = ev_ms(ctx, 0, 5);
}

// ---- full (encrypted-share) mode: hybrid.hip (elgamal.rs:134-193, committee.rs:164-172, 282-286)
// Items (dealer i, recipient q, w) at (i * n + q) * 2 + w: w = 0 the randomness s', w = 1 the share s.
// pk_host (optional): the same keys on the host.  Member keys outlive a ceremony (procedure_keys.rs),
// so their decoded points and comb tables are kept in the arena and rebuilt only when the keys
// differ from the last build's (compared byte for byte).
// K = pk_q * r comes from one of two combs of the recipient keys, each with its own arena buffers and its
// own cache key (a kind's cache never passes for the other's): kind 1, radix 2^DKG_KEY_COMB_BITS
// (hy.*, k_enc_mul: both products in one kernel), or kind 2, the batches' signed radix-16 combs
// (hy16.*: k_benc_tab, then e1 = g r by fixed_base and K by k_benc_mul with D rows per key).
// ctx->key_comb forces a kind; at 0 the kind is 1 unless the caller lets the cost rule choose
// (choose: the sharded full calls, where a key serves 2 D items and a cold 2^10 build outweighs them).
// Returns the keys' decode mask [n] of the kind used (device).
// full.*: the kernels' device times of a ceremony's serialised encrypt + decrypt, collected after its sync by
// every full-mode ceremony, so that a phase it did not time (chunk streams, or a verify-only ceremony without
// encryption) reads -1.
enum { FP_ENC_MUL, FP_ENC_ENCODE, FP_ENC_SYM, FP_DEC_DECODE, FP_DEC_MUL, FP_DEC_ENCODE, FP_DEC_SYM };
const PhaseRow FULL_PHASES[] = {{"enc_mul", 1u << FP_ENC_MUL},       {"enc_encode", 1u << FP_ENC_ENCODE},
                                {"enc_sym", 1u << FP_ENC_SYM},       {"dec_decode", 1u << FP_DEC_DECODE},
                                {"dec_mul", 1u << FP_DEC_MUL},       {"dec_encode", 1u << FP_DEC_ENCODE},
                                {"dec_sym", 1u << FP_DEC_SYM}};
const uint8_t* encrypt_device(dkg_ctx* ctx, size_t D, size_t n, const uint32_t* pkc, const uint32_t* s,
                              const uint32_t* sp, const uint32_t* r, uint32_t* e1, uint32_t* ct,
                              hipStream_t st = nullptr, const uint8_t* pk_host = nullptr, bool choose = false) {
  const size_t items = 2 * D * n;
  if (!st) st = ctx->stream;
  auto same = [&](const std::vector<uint8_t>& k) {
    return pk_host && k.size() == 32 * n && memcmp(k.data(), pk_host, 32 * n) == 0;
  };
  const bool cached10 = same(ctx->key_tabs_pk), cached16 = same(ctx->key_tabs16_pk);
  const int kind = ctx->key_comb ? ctx->key_comb : choose ? dkg_key_comb_choice(n, 2 * D, cached10, cached16) : 1;
  ctx->last_key_comb = kind;
  std::vector<uint8_t>& held = kind == 1 ? ctx->key_tabs_pk : ctx->key_tabs16_pk;
  uint32_t* pk_ext = buf<uint32_t>(ctx, kind == 1 ? "hy.pk_ext" : "hy16.pk_ext", PTB * n);
  uint8_t* pk_ok = buf<uint8_t>(ctx, kind == 1 ? "hy.pk_ok" : "hy16.pk_ok", n);
  uint32_t* tabs = kind == 1 ? buf<uint32_t>(ctx, "hy.tabs", 4 * dkgk::key_comb_words() * n)
                             : buf<uint32_t>(ctx, "hy16.tabs", 4 * dkgk::benc_tab_words() * n);
  if (!(kind == 1 ? cached10 : cached16)) {
    held.clear();  // invalid until this build is queued
    dkgk::decode_points(pkc, n, pk_ext, n, pk_ok, st);
    // one comb per recipient key: r * pk_q is fixed-base
    if (kind == 1) build_combs(ctx, 1, pk_ext, n, 0, tabs, st, n);
    else dkgk::benc_tab(n, pk_ext, n, tabs, st);
    if (pk_host) held.assign(pk_host, pk_host + 32 * n);
  }
  uint32_t* R = buf<uint32_t>(ctx, "hy.R", PTB * items);
  uint32_t* K = buf<uint32_t>(ctx, "hy.K", PTB * items);
  uint32_t* Kc = buf<uint32_t>(ctx, "hy.Kc", 32 * items);
  // phase events (serialised runs, nsub == 1): the bench's per-kernel roofline of full mode
  const bool tm = ctx->nsub == 1;
  if (tm) phase_mark(ctx, st, "full", -1);
  if (kind == 1) {
    dkgk::enc_mul(D, n, r, ctx->tab_gw, tabs, R, K, st);
  } else {
    dkgk::fixed_base(items, r, ctx->tab_gw, R, st);         // e1 = G::generator() * r  (elgamal.rs:141)
    dkgk::benc_mul(n, n, D, r, tabs, K, items, st);         // key = pk * r  (elgamal.rs:138-140)
  }
  if (tm) phase_mark(ctx, st, "full", FP_ENC_MUL);
  dkgk::encode_points(R, items, items, e1, st);
  dkgk::encode_points(K, items, items, Kc, st);
  if (tm) phase_mark(ctx, st, "full", FP_ENC_ENCODE);
  dkgk::sym_xor(D, n, Kc, false, ct, const_cast<uint32_t*>(s), const_cast<uint32_t*>(sp), st);
  if (tm) phase_mark(ctx, st, "full", FP_ENC_SYM);
  check_launch(ctx);
  return pk_ok;
}

// Receivers' side: item_ok[item] = e1 decodes; dealer_ok_out[i] = all of dealer i's items decode (a
// broadcast that does not deserialize is missing data, committee.rs:331-335).
void decrypt_device(dkg_ctx* ctx, size_t D, size_t n, const uint32_t* sk, const uint32_t* e1, const uint32_t* ct,
                    uint32_t* s, uint32_t* sp, uint8_t* item_ok, uint8_t* dealer_ok_out, hipStream_t st = nullptr) {
  const size_t items = 2 * D * n;
  if (!st) st = ctx->stream;
  uint32_t* R = buf<uint32_t>(ctx, "hy.R", PTB * items);
  uint32_t* K = buf<uint32_t>(ctx, "hy.K", PTB * items);
  uint32_t* Kc = buf<uint32_t>(ctx, "hy.Kc", 32 * items);
  const bool tm = ctx->nsub == 1;
  if (tm) phase_mark(ctx, st, "full", -1);
  dkgk::decode_points(e1, items, R, items, item_ok, st);
  if (tm) phase_mark(ctx, st, "full", FP_DEC_DECODE);
  const size_t tw = dkgk::dec_mul_table_words(D, n);
  dkgk::dec_mul(D, n, sk, R, K, st, tw ? buf<uint32_t>(ctx, "hy.dec_tab", 4 * tw) : nullptr);
  if (tm) phase_mark(ctx, st, "full", FP_DEC_MUL);
  dkgk::encode_points(K, items, items, Kc, st);
  if (tm) phase_mark(ctx, st, "full", FP_DEC_ENCODE);
  dkgk::sym_xor(D, n, Kc, true, const_cast<uint32_t*>(ct), s, sp, st);
  if (tm) phase_mark(ctx, st, "full", FP_DEC_SYM);
  if (dealer_ok_out) dkgk::dealer_ok(D, 2 * n, item_ok, dealer_ok_out, st);
  check_launch(ctx);
}

// ---- full mode for batches (hybrid_batch.hip): ceremony c's recipients own keys c*n .. c*n + n-1.
// The hybrid stage runs in chunks of ceremonies so that its scratch -- the extended-form R and K, the
// K encodings, the decoded keys and their radix-16 combs, the decryption's odd-multiple table -- does
// not grow with B (10,000 x 64 unchunked: 26 GB of R / K / Kc and 52 GB of combs).
constexpr size_t BFULL_SCRATCH_BYTES = (size_t)2 << 30;  // automatic chunk: R + K + Kc + keys + combs within 2 GiB
enum {
  BF_ENC_DECODE, BF_ENC_TAB, BF_ENC_E1, BF_ENC_MUL, BF_ENC_ENCODE, BF_ENC_SYM,
  BF_DEC_DECODE, BF_DEC_MUL, BF_DEC_ENCODE, BF_DEC_SYM, BF_PHASES
};
// bfull.*: the summed device times of a call's hybrid kernels over all chunks; a phase it did not run reads -1
const PhaseRow BF_ROWS[BF_PHASES] = {
    {"enc_decode", 1u << BF_ENC_DECODE}, {"enc_tab", 1u << BF_ENC_TAB},       {"enc_e1", 1u << BF_ENC_E1},
    {"enc_mul", 1u << BF_ENC_MUL},       {"enc_encode", 1u << BF_ENC_ENCODE}, {"enc_sym", 1u << BF_ENC_SYM},
    {"dec_decode", 1u << BF_DEC_DECODE}, {"dec_mul", 1u << BF_DEC_MUL},       {"dec_encode", 1u << BF_DEC_ENCODE},
    {"dec_sym", 1u << BF_DEC_SYM}};

size_t bfull_chunk_size(const dkg_ctx* ctx, size_t B, size_t n) {
  const size_t items = 2 * n * n;
  const size_t per = items * (2 * PTB + 32) + n * (PTB + 4 * dkgk::benc_tab_words());
  // automatic: within the scratch budget, and the chunk's decryption one launch under the table cap
  const size_t fit = std::min(BFULL_SCRATCH_BYTES / per, dkgk::bdec_launch_waves() / (2 * n * ((n + 63) / 64)));
  const size_t c = ctx->bfull_chunk ? ctx->bfull_chunk : std::max<size_t>(1, fit);
  return std::min(c, B);
}

// Dealers' side: pkc [B*n][8] key encodings, s / sp [B*n][n][8], r [B*n][n][2][8] -> e1, ct
// [B*n][n][2][8]; pk_ok [B*n] = the key decodes.  All on ctx->stream.
void encrypt_batch_device(dkg_ctx* ctx, size_t B, size_t n, const uint32_t* pkc, const uint32_t* s, const uint32_t* sp,
                          const uint32_t* r, uint32_t* e1, uint32_t* ct, uint8_t* pk_ok) {
  hipStream_t st = ctx->stream;
  const size_t chunk = bfull_chunk_size(ctx, B, n);
  const size_t mk = chunk * n, mi = 2 * mk * n;
  uint32_t* pk_ext = buf<uint32_t>(ctx, "bf.pk_ext", PTB * mk);
  uint32_t* tab = buf<uint32_t>(ctx, "bf.tab", 4 * dkgk::benc_tab_words() * mk);
  uint32_t* R = buf<uint32_t>(ctx, "bf.R", PTB * mi);
  uint32_t* K = buf<uint32_t>(ctx, "bf.K", PTB * mi);
  uint32_t* Kc = buf<uint32_t>(ctx, "bf.Kc", 32 * mi);
  phase_mark(ctx, st, "bfull", -1);
  for (size_t c0 = 0; c0 < B; c0 += chunk) {
    const size_t Bc = std::min(chunk, B - c0), keys = Bc * n, items = 2 * keys * n;
    const size_t k0 = c0 * n, p0 = k0 * n, i0 = 2 * p0;  // first key / (dealer, recipient) pair / item
    dkgk::decode_points(pkc + 8 * k0, keys, pk_ext, keys, pk_ok + k0, st);
    phase_mark(ctx, st, "bfull", BF_ENC_DECODE);
    dkgk::benc_tab(keys, pk_ext, keys, tab, st);
    phase_mark(ctx, st, "bfull", BF_ENC_TAB);
    dkgk::fixed_base(items, r + 8 * i0, ctx->tab_gw, R, st);  // e1 = G::generator() * r  (elgamal.rs:141)
    phase_mark(ctx, st, "bfull", BF_ENC_E1);
    dkgk::benc_mul(keys, n, n, r + 8 * i0, tab, K, items, st);   // key = pk * r  (elgamal.rs:138-140)
    phase_mark(ctx, st, "bfull", BF_ENC_MUL);
    dkgk::encode_points(R, items, items, e1 + 8 * i0, st);
    dkgk::encode_points(K, items, items, Kc, st);
    phase_mark(ctx, st, "bfull", BF_ENC_ENCODE);
    dkgk::sym_xor(keys, n, Kc, false, ct + 8 * i0, const_cast<uint32_t*>(s) + 8 * p0,
                  const_cast<uint32_t*>(sp) + 8 * p0, st);
    phase_mark(ctx, st, "bfull", BF_ENC_SYM);
  }
  check_launch(ctx);
}

// Receivers' side: sk [B*n][8]; item_ok [B*n][n][2] = e1 decodes; dealer_ok_out (may be null) [B*n].
void decrypt_batch_device(dkg_ctx* ctx, size_t B, size_t n, const uint32_t* sk, const uint32_t* e1, const uint32_t* ct,
                          uint32_t* s, uint32_t* sp, uint8_t* item_ok, uint8_t* dealer_ok_out) {
  hipStream_t st = ctx->stream;
  const size_t chunk = bfull_chunk_size(ctx, B, n);
  const size_t mk = chunk * n, mi = 2 * mk * n;
  uint32_t* R = buf<uint32_t>(ctx, "bf.R", PTB * mi);
  uint32_t* K = buf<uint32_t>(ctx, "bf.K", PTB * mi);
  uint32_t* Kc = buf<uint32_t>(ctx, "bf.Kc", 32 * mi);
  uint32_t* T = buf<uint32_t>(ctx, "bf.dec_tab", 4 * dkgk::bdec_mul_table_words(mk, n));
  phase_mark(ctx, st, "bfull", -1);
  for (size_t c0 = 0; c0 < B; c0 += chunk) {
    const size_t Bc = std::min(chunk, B - c0), keys = Bc * n, items = 2 * keys * n;
    const size_t k0 = c0 * n, p0 = k0 * n, i0 = 2 * p0;
    dkgk::decode_points(e1 + 8 * i0, items, R, items, item_ok + i0, st);
    phase_mark(ctx, st, "bfull", BF_DEC_DECODE);
    dkgk::bdec_mul(keys, n, sk + 8 * k0, R, K, items, T, st);  // committee.rs:282-286
    phase_mark(ctx, st, "bfull", BF_DEC_MUL);
    dkgk::encode_points(K, items, items, Kc, st);
    phase_mark(ctx, st, "bfull", BF_DEC_ENCODE);
    dkgk::sym_xor(keys, n, Kc, true, const_cast<uint32_t*>(ct) + 8 * i0, s + 8 * p0, sp + 8 * p0, st);
    phase_mark(ctx, st, "bfull", BF_DEC_SYM);
  }
  if (dealer_ok_out) dkgk::dealer_ok(B * n, 2 * n, item_ok, dealer_ok_out, st);
  check_launch(ctx);
}

// ---- complaint proofs (dl_equality/zkp.rs, broadcast.rs:50-135, 181-283)
// Cold path (one proof per complaint): the group work goes to the GPU as batched MSMs (k_msm), the
// Fiat-Shamir hashes, ChaCha20 and scalar arithmetic run on the host.
// B MSMs of N terms: scalars / points host [B][N][32] -> out [B][32]; ok[b] = every point decodes.
void msm_host(dkg_ctx* ctx, size_t B, size_t N, const uint8_t* scalars, const uint8_t* points, uint8_t* out,
              std::vector<uint8_t>& ok) {
  ok.assign(B, 1);
  if (!B) return;
  uint32_t* sc = upload_scalars(ctx, "cp_sc", scalars, B * N);
  uint32_t* pc = buf<uint32_t>(ctx, "cp_pc", 32 * B * N);
  uint32_t* pe = buf<uint32_t>(ctx, "cp_pe", PTB * B * N);
  uint8_t* pok = buf<uint8_t>(ctx, "cp_ok", B * N);
  h2d(ctx, pc, points, 32 * B * N);
  dkgk::decode_points(pc, B * N, pe, B * N, pok, ctx->stream);
  uint32_t* oe = buf<uint32_t>(ctx, "cp_oe", PTB * B);
  uint32_t* oc = buf<uint32_t>(ctx, "cp_oc", 32 * B);
  uint32_t* mt = buf<uint32_t>(ctx, "msm_tab", 4 * 15 * PT_WORDS_H * B * N);
  dkgk::msm_batch(B, N, sc, pe, B * N, mt, oe, ctx->stream);
  dkgk::encode_points(oe, B, B, oc, ctx->stream);
  check_launch(ctx);
  std::vector<uint8_t> okh(B * N);
  d2h(ctx, okh.data(), pok, B * N);
  d2h(ctx, out, oc, 32 * B);
  sync(ctx);
  for (size_t b = 0; b < B; b++)
    for (size_t k = 0; k < N; k++) ok[b] &= okh[b * N + k];
}

dkgh::Zl zl32(const uint8_t* p) { return dkgh::zl_from_bits(p); }  // a scalar off the wire
void put32(std::vector<uint8_t>& v, const uint8_t* p) { v.insert(v.end(), p, p + 32); }
void putzl(std::vector<uint8_t>& v, const dkgh::Zl& z) {
  uint8_t b[32];
  dkgh::zl_to_bytes(b, z);
  put32(v, b);
}

// Scalar::hash_from_bytes::<Blake2b> (groups.rs:50-52) of ChallengeContext b1||b2||p1||p2||a1||a2
// (challenge_context.rs:14-41)
dkgh::Zl dleq_challenge(const uint8_t* b1, const uint8_t* b2, const uint8_t* p1, const uint8_t* p2, const uint8_t* a1,
                        const uint8_t* a2) {
  uint8_t buf_[192], h[64];
  const uint8_t* parts[6] = {b1, b2, p1, p2, a1, a2};
  for (int i = 0; i < 6; i++) memcpy(buf_ + 32 * i, parts[i], 32);
  dkgh::blake2b(h, 64, buf_, 192);
  return dkgh::zl_from_bytes_wide(h, 64);
}

// SymmetricKey::process + Scalar::from_bytes (from_bits, reduced) of a 32-byte ciphertext
dkgh::Zl sym_scalar(const uint8_t K[32], const uint8_t ct[32]) {
  uint8_t h[64], m[32];
  dkgh::blake2b(h, 64, K, 32);
  dkgh::chacha20_ietf_xor(m, ct, 32, h, h + 32);
  m[31] &= 0x7f;
  return zl32(m);
}

std::vector<uint8_t> index_powers(uint32_t j, size_t N) {  // from_u64(j).exp_iter().take(N)
  std::vector<uint8_t> out;
  dkgh::Zl x = dkgh::zl_from_u64(j), p = dkgh::zl_from_u64(1);
  for (size_t k = 0; k < N; k++) {
    putzl(out, p);
    p = dkgh::zl_mul(p, x);
  }
  return out;
}

int need_env(dkg_ctx* ctx) {
  if (!ctx->have_h) {
    ctx->err = "dkg_env_init has not been called (commitment key unknown)";
    return DKG_E_ARG;
  }
  return DKG_OK;
}

// The argument prologue of the entry points that need the commitment key, one ceremony's and a
// batch's alike: the environment is set, (t, n) are admissible and none of `required` is null.
int ceremony_args(dkg_ctx* ctx, size_t n, size_t t, std::initializer_list<const void*> required) {
  const int rc = need_env(ctx);
  if (rc) return rc;
  if (dkg_env_check(t, n) != DKG_OK) return DKG_E_ARG;
  for (const void* p : required)
    if (!p) return DKG_E_ARG;
  return DKG_OK;
}

// ---- round-2 complaints as device batches (complaints.hip)
// Does an accused dealer with `count` complaints get the difference tables of its row (every P_i(j),
// verify_device without checks) instead of one Horner walk per complaint?  Both are one dependent
// chain however many complaints there are (the walks of all complaints run side by side, and so do
// the tables of all accused rows), so what decides is the chains' lengths, not the work:
//   Horner: N steps of nb doublings, one addition per index bit some lane of the wave has set
//           (about the bit length of `count` + 1 for a dealer accused by receivers 1..count), + 1;
//   tables: N binomial steps and n stepping steps.
// The per-step latencies are fitted to profiles/complaints_eval_ab.txt (n = 1024, t = 511: the tables
// win at every count, 11.3-11.6 ms against 23.0-39.6 ms per call at 1-1,023 complaints; n = 1024, t = 3:
// Horner wins at every count, 3.2-3.5 against 7.0-7.2 ms; n = 64 and 256 with t = (n-1)/2 in between).
bool complaint_tables_pay(size_t n, size_t N, size_t count) {
  if (N < 2) return false;  // a constant polynomial: P_i(j) = E_i0
  int nb = 1, cb = 1;
  while ((n >> nb) != 0) nb++;
  while ((count >> cb) != 0) cb++;
  const double horner_us = 3.6 * (double)N * (nb + std::min(nb, cb + 1) + 1);
  const double tables_us = 13.0 * (double)N + 3.7 * (double)n;
  return tables_us < horner_us;
}

// Field multiplication of k_pair_eval when dkg_ctx_set_field_mode leaves the choice open: 1 column sums
// (dkgk_ilp), 0 product scanning (A/B in profiles/pairs_time.json).
#ifndef DKG_PAIR_ILP
#define DKG_PAIR_ILP 1
#endif

// The fold multipliers of a plan as the digit records recv_mul_long reads (receivers.hip): the NAF of
// mult[s] in out[fold_record(0, stages, s) ..], stages * FOLD_DIG_WORDS words in all.
void fold_records(const dkg_receiver_plan& p, uint32_t* out) {
  for (uint32_t s = 0; s < p.stages; s++) {
    uint32_t* d = out + fold_record(0, p.stages, s);
    d[16] = (uint32_t)dkgh::naf256(p.mult[s], d, d + 8, nullptr);
  }
}

// One wave per (row, index) item (receivers.hip k_pair_eval) in the shape of dkg_pair_eval_shape under
// ctx->receiver_chunk.  Item b < cnt: c = dlist[b] (b itself with a null dlist), row dcrow[c] - 1 of Cext
// (element row * N + k, stride), index dxs[c] = hx[b] (1-based; hx on the host, per ITEM).  The fold's
// multipliers are dkg_receiver_plan_for's for the forced chunk L, as signed digits (fold_records), one
// [S][FOLD_DIG_WORDS] record per DISTINCT index of the call (cached on the ctx).  R[c][40].  The staging
// vectors `slot` and `dig` are the caller's to keep until it has synchronised.
struct PairStage {
  std::vector<uint32_t> xs, slot, dig;
};
void pair_eval_launch(dkg_ctx* ctx, size_t t, size_t cnt, const uint32_t* dlist, const uint32_t* hx,
                      const uint32_t* dxs, const uint32_t* dcrow, const uint32_t* Cext, size_t stride, uint32_t* R,
                      PairStage& ps) {
  if (!cnt) return;
  const size_t N = t + 1;
  uint32_t L, G, S;
  if (dkg_pair_eval_shape(t, ctx->receiver_chunk, &L, &G, &S) != DKG_OK) {
    ctx->err = "pair evaluation: the forced receiver chunk needs more than 64 lanes";
    throw Fail{DKG_E_ARG};
  }
  ctx->last_receiver_chunk = (int)L;
  dkgh::distinct_places(cnt, hx, ps.xs, ps.slot);
  const size_t rec_words = fold_record(1, S, 0);
  ps.dig.assign(std::max<size_t>(1, ps.xs.size() * rec_words), 0);
  for (size_t m = 0; m < ps.xs.size() && S; m++) {
    const uint32_t x = ps.xs[m];
    const std::array<size_t, 3> key = {t, x, L};
    auto it = ctx->pair_digits.find(key);
    if (it == ctx->pair_digits.end()) {
      dkg_receiver_plan p;
      if (dkg_receiver_plan_for(x, t, x, (int)L, &p) != DKG_OK || p.stages != S) {
        ctx->err = "pair evaluation: no plan for the index";
        throw Fail{DKG_E_ARG};
      }
      std::vector<uint32_t> rec(rec_words, 0);
      fold_records(p, rec.data());
      if (ctx->pair_digits.size() >= 65536) ctx->pair_digits.clear();
      it = ctx->pair_digits.emplace(key, std::move(rec)).first;
    }
    memcpy(&ps.dig[m * rec_words], it->second.data(), 4 * rec_words);
  }
  uint32_t* dslot = upload_words(ctx, "pe_slot", ps.slot);
  uint32_t* ddig = upload_words(ctx, "pe_dig", ps.dig);
  const bool ilp = ctx->fe_mode == 2 || (ctx->fe_mode == 0 && DKG_PAIR_ILP);
  (ilp ? dkgk_ilp::pair_eval : dkgk::pair_eval)(cnt, dlist, dxs, dcrow, dslot, Cext, stride, N, L, G, S, ddig, R,
                                                ctx->stream);
}

// P_row(x) = sum_k x^k C_row[k] for C (row, index) items: per row, the difference tables of that row
// or one Horner walk per item (ctx->complaint_eval; automatic: complaint_tables_pay by the row's item
// count).  Mode 4 sends every item to the wave evaluator (pair_eval_launch), which writes Rh in the walk's
// place.  index / row (host) and dindex / drow (device) [C]: 1-based, index within 1..n, row within
// 1..nrows; Cc [nrows][N][8] compressed and Cext (stride nrows * N) decoded commitments on the device.
// An (row, index) pair listed again takes a further table row of its own, so that the table path
// serves every item of a row it is chosen for.  Out: dridx [C] (bit 31: element of Rt, else of Rh),
// Rh, Rt, scale as k_cv_check reads them.  Work is queued on ctx->stream; the staging vectors live
// in `ev`, which the caller keeps until it has synchronised.
struct ComplaintEvals {
  std::vector<uint32_t> rows, hl, ridx, hx;
  PairStage ps;
  const uint32_t *dridx = nullptr, *Rh = nullptr, *Rt = nullptr, *scale = nullptr;
};
void complaint_evals(dkg_ctx* ctx, size_t n, size_t t, size_t nrows, size_t C, const uint32_t* index,
                     const uint32_t* row, const uint32_t* dindex, const uint32_t* drow, const uint32_t* Cc,
                     const uint32_t* Cext, ComplaintEvals& ev) {
  const size_t N = t + 1;
  hipStream_t st = ctx->stream;
  std::vector<size_t> count(nrows, 0);
  for (size_t c = 0; c < C; c++) count[row[c] - 1]++;
  std::map<std::pair<uint32_t, uint32_t>, uint32_t> seen;   // (row, index) -> occurrences so far
  std::map<std::pair<uint32_t, uint32_t>, uint32_t> rowof;  // (row, occurrence) -> table row
  std::vector<uint32_t>&rows = ev.rows, &hl = ev.hl, &ridx = ev.ridx;
  ridx.resize(C);
  for (size_t c = 0; c < C; c++) {
    const uint32_t i = row[c], j = index[c];
    const bool tables = N >= 2 && (ctx->complaint_eval == 2 ||
                                   (ctx->complaint_eval == 0 && complaint_tables_pay(n, N, count[i - 1])));
    if (!tables) {
      hl.push_back((uint32_t)c);
      ridx[c] = (uint32_t)c;
      continue;
    }
    const uint32_t m = seen[{i, j}]++;
    auto it = rowof.find({i, m});
    if (it == rowof.end()) {
      it = rowof.emplace(std::make_pair(i, m), (uint32_t)rows.size()).first;
      rows.push_back(i);
    }
    if (((size_t)it->second + 1) * n >= ((size_t)1 << 31)) {
      ctx->err = "complaints_verify: too many table rows";
      throw Fail{DKG_E_ARG};
    }
    ridx[c] = 0x80000000u | (uint32_t)((size_t)it->second * n + (j - 1));
  }
  uint32_t* dridx = buf<uint32_t>(ctx, "cv_ridx", 4 * C);
  h2d(ctx, dridx, ridx.data(), 4 * C);
  uint32_t* Rh = buf<uint32_t>(ctx, "cv_Rh", PTB * C);
  if (!hl.empty()) {
    uint32_t* dhl = buf<uint32_t>(ctx, "cv_hl", 4 * hl.size());
    h2d(ctx, dhl, hl.data(), 4 * hl.size());
    if (ctx->complaint_eval == 4) {
      ev.hx.resize(hl.size());
      for (size_t k = 0; k < hl.size(); k++) ev.hx[k] = index[hl[k]];
      pair_eval_launch(ctx, t, hl.size(), dhl, ev.hx.data(), dindex, drow, Cext, nrows * N, Rh, ev.ps);
    } else {
      int nb = 1;
      while ((n >> nb) != 0) nb++;
      dkgk::cmp_horner(hl.size(), dhl, dindex, drow, Cext, nrows * N, N, nb, Rh, st);
    }
  }
  if (!rows.empty()) {
    const size_t D = rows.size();
    uint32_t* Trows = buf<uint32_t>(ctx, "cv_Trows", 32 * D * N);
    for (size_t r = 0; r < D; r++)
      HCK(hipMemcpyAsync(Trows + 8 * N * r, Cc + 8 * N * (size_t)(rows[r] - 1), 32 * N, hipMemcpyDeviceToDevice, st));
    VerifySeg g{2, D, 0, Trows, nullptr, nullptr, nullptr};
    verify_device(ctx, n, t, &g, 1, false, "cv");
    ev.Rt = ctx->last_R;
    ev.scale = ctx->last_scale;
  }
  ev.dridx = dridx;
  ev.Rh = Rh;
}

// The announcements of C round-2 complaints' proofs (dl_equality/zkp.rs:60-63): a1 = g r - pk c (comb +
// one-base walk), a2 = e1 r - K c (Straus), both encoded, with p12 and the decode mask ppok [5C] of
// the complaints' points as k_cv_check / k_cv_final read them.  Device: party [C] the accuser's 1-based
// row of pk; enc [C][128], proofs [C][192].  One ceremony and a batch share the cv_* buffers.
struct Announcements {
  const uint32_t *p12, *a1c, *a2c;
  const uint8_t* ppok;
};
Announcements complaint_announcements(dkg_ctx* ctx, size_t C, const uint32_t* party, const uint32_t* dpk,
                                      const uint32_t* denc, const uint32_t* dprf, hipStream_t st) {
  // scalars, the points to decode, SymmetricKey::process of both ciphertexts
  uint32_t* Pc = buf<uint32_t>(ctx, "cv_Pc", 32 * 5 * C);
  uint32_t* rs = buf<uint32_t>(ctx, "cv_rs", 32 * 2 * C);
  uint32_t* nc = buf<uint32_t>(ctx, "cv_nc", 32 * 2 * C);
  uint32_t* p12 = buf<uint32_t>(ctx, "cv_p12", 32 * 2 * C);
  uint32_t* bp1 = buf<uint32_t>(ctx, "cv_bp1", 4 * 2 * C);
  uint32_t* bp2 = buf<uint32_t>(ctx, "cv_bp2", 4 * 2 * C);
  uint32_t* bq2 = buf<uint32_t>(ctx, "cv_bq2", 4 * 2 * C);
  dkgk::cv_prep(C, party, dpk, denc, dprf, Pc, rs, nc, p12, bp1, bp2, bq2, st);
  uint32_t* Pext = buf<uint32_t>(ctx, "cv_Pext", PTB * 5 * C);
  uint8_t* ppok = buf<uint8_t>(ctx, "cv_Ppok", 5 * C);
  dkgk::decode_points(Pc, 5 * C, Pext, 5 * C, ppok, st);
  uint32_t* T = buf<uint32_t>(ctx, "cv_T", 4 * dkgk::cmp_ladder_table_words(2 * C));
  uint32_t* S1 = buf<uint32_t>(ctx, "cv_S1", PTB * 2 * C);
  uint32_t* S2 = buf<uint32_t>(ctx, "cv_S2", PTB * 2 * C);
  uint32_t* G = buf<uint32_t>(ctx, "cv_G", PTB * 2 * C);
  dkgk::cmp_ladder(2 * C, false, bp1, nullptr, nc, nullptr, Pext, 5 * C, T, S1, st);
  dkgk::cmp_ladder(2 * C, true, bp2, bq2, rs, nc, Pext, 5 * C, T, S2, st);
  dkgk::fixed_base(2 * C, rs, ctx->tab_gw, G, st);
  dkgk::add_points(2 * C, S1, G, 2 * C, S1, st);
  uint32_t* a1c = buf<uint32_t>(ctx, "cv_a1c", 32 * 2 * C);
  uint32_t* a2c = buf<uint32_t>(ctx, "cv_a2c", 32 * 2 * C);
  dkgk::encode_points(S1, 2 * C, 2 * C, a1c, st);
  dkgk::encode_points(S2, 2 * C, 2 * C, a2c, st);
  return {p12, a1c, a2c, ppok};
}

// MisbehavingPartiesRound1::verify (broadcast.rs:50-99) for C complaints of one ceremony.  Device: dpk
// [n][8] member keys, Ec [n][N][8] commitments; host: accuser / accused (1-based, validated by the
// caller), fetched1 (may be null), enc [C][128], proofs [C][192].  verdict [C] on the host; rowok_host
// (may be null) [n] = E row i decodes.  Ends synchronised.
void complaints_verify_core(dkg_ctx* ctx, size_t n, size_t t, size_t C, const uint32_t* accuser,
                            const uint32_t* accused, const uint32_t* dpk, const uint32_t* Ec, const uint8_t* fetched1,
                            const uint8_t* enc, const uint8_t* proofs, int32_t* verdict, uint8_t* rowok_host) {
  const size_t N = t + 1;
  hipStream_t st = ctx->stream;
  // every row decoded once: the rows' validity for the qualified set, and the Horner walks' input
  uint32_t* Eext = buf<uint32_t>(ctx, "cv_Eext", PTB * n * N);
  uint8_t* epok = buf<uint8_t>(ctx, "cv_Epok", n * N);
  uint8_t* rowok = buf<uint8_t>(ctx, "cv_rowok", n);
  dkgk::decode_points(Ec, n * N, Eext, n * N, epok, st);
  dkgk::dealer_ok(n, N, epok, rowok, st);
  if (rowok_host) d2h(ctx, rowok_host, rowok, n);
  if (!C) {
    check_launch(ctx);
    sync(ctx);
    return;
  }
  uint32_t* dacc = buf<uint32_t>(ctx, "cv_accuser", 4 * C);
  uint32_t* dacd = buf<uint32_t>(ctx, "cv_accused", 4 * C);
  uint32_t* denc = buf<uint32_t>(ctx, "cv_enc", 128 * C);
  uint32_t* dprf = buf<uint32_t>(ctx, "cv_proofs", 192 * C);
  h2d(ctx, dacc, accuser, 4 * C);
  h2d(ctx, dacd, accused, 4 * C);
  h2d(ctx, denc, enc, 128 * C);
  h2d(ctx, dprf, proofs, 192 * C);
  const uint8_t* dfet = upload_mask(ctx, "cv_fetched", fetched1, n);
  const Announcements an = complaint_announcements(ctx, C, dacc, dpk, denc, dprf, st);
  // P_i(j): per accused dealer, the difference tables of its row or one Horner walk per complaint
  ComplaintEvals ev;
  complaint_evals(ctx, n, t, n, C, accuser, accused, dacc, dacd, Ec, Eext, ev);
  const uint32_t *dridx = ev.dridx, *Rh = ev.Rh, *Rt = ev.Rt, *scale = ev.scale;
  uint8_t* eq = buf<uint8_t>(ctx, "cv_eq", 2 * C);
  dkgk::cv_check(C, dacc, an.p12, dridx, Rh, Rt, scale, ctx->tab_gw, ctx->tab_hw, eq, st);
  int32_t* dver = buf<int32_t>(ctx, "cv_verdict", 4 * C);
  dkgk::cv_final(C, dacc, dacd, dpk, denc, dprf, an.a1c, an.a2c, an.ppok, rowok, dfet, eq, dver, st);
  check_launch(ctx);
  d2h(ctx, verdict, dver, 4 * C);
  sync(ctx);  // the staging vectors (ev) live until here
}

// C complaints' arguments: with C > 0 the index arrays and `payload` (what the complaints carry, and
// where their verdicts go) are present, and the 1-based party indices lie within 1..n
bool complaint_args_ok(size_t n, size_t C, const uint32_t* accuser, const uint32_t* accused,
                       std::initializer_list<const void*> payload) {
  if (!C) return true;
  if (!accuser || !accused) return false;
  for (const void* p : payload)
    if (!p) return false;
  for (size_t c = 0; c < C; c++)
    if (accuser[c] < 1 || accuser[c] > n || accused[c] < 1 || accused[c] > n) return false;
  return true;
}

// dissent[j] = the dealers receiver j rejected in the ceremony just run (dec2 on the device) without a
// proven complaint of its own against them among the C
void complaint_dissent(dkg_ctx* ctx, size_t n, size_t C, const uint32_t* accuser, const uint32_t* accused,
                       const int32_t* verdict, int32_t* dissent) {
  std::vector<uint8_t> d2(n * n);
  d2h(ctx, d2.data(), buf<uint8_t>(ctx, "dec2", n * n), n * n);
  sync(ctx);
  std::vector<uint8_t> proven(n * n, 0);  // [accused][accuser]
  for (size_t c = 0; c < C; c++)
    if (verdict[c] == 0) proven[(size_t)(accused[c] - 1) * n + (accuser[c] - 1)] = 1;
  for (size_t j = 0; j < n; j++) {
    int32_t v = 0;
    for (size_t i = 0; i < n; i++) v += d2[i * n + j] == DKG_REJECT && !proven[i * n + j];
    dissent[j] = v;
  }
}

// ---- round-4 complaints as a device batch (complaints.hip, k_c3_*)
// MisbehavingPartiesRound3::verify (broadcast.rs:104-144) as Phases<Phase4>::proceed applies it
// (committee.rs:636-670) for C complaints of one ceremony.  Device: EA [2n][N][8], the E rows then the A
// rows; host: accuser / accused (1-based, validated by the caller), share / randomness [C][32],
// qualified / fetched3 [n] (may be null = all 1).  verdict [C] on the host; rowok_host (may be null)
// [2n] = the row decodes.  Ends synchronised.
void complaints3_core(dkg_ctx* ctx, size_t n, size_t t, size_t C, const uint32_t* accuser, const uint32_t* accused,
                      const uint8_t* share, const uint8_t* randomness, const uint32_t* EA, const uint8_t* qualified,
                      const uint8_t* fetched3, int32_t* verdict, uint8_t* rowok_host) {
  const size_t N = t + 1;
  hipStream_t st = ctx->stream;
  // both rows of every dealer decoded once: the rows' validity, and the Horner walks' input
  uint32_t* EAext = buf<uint32_t>(ctx, "c3_EAext", PTB * 2 * n * N);
  uint8_t* pok = buf<uint8_t>(ctx, "c3_pok", 2 * n * N);
  uint8_t* rowok = buf<uint8_t>(ctx, "c3_rowok", 2 * n);
  dkgk::decode_points(EA, 2 * n * N, EAext, 2 * n * N, pok, st);
  dkgk::dealer_ok(2 * n, N, pok, rowok, st);
  if (rowok_host) d2h(ctx, rowok_host, rowok, 2 * n);
  if (!C) {
    check_launch(ctx);
    sync(ctx);
    return;
  }
  uint32_t* dacc = buf<uint32_t>(ctx, "c3_accuser", 4 * C);
  uint32_t* dacd = buf<uint32_t>(ctx, "c3_accused", 4 * C);
  uint32_t* dsh = buf<uint32_t>(ctx, "c3_share", 32 * C);
  uint32_t* drn = buf<uint32_t>(ctx, "c3_rand", 32 * C);
  h2d(ctx, dacc, accuser, 4 * C);
  h2d(ctx, dacd, accused, 4 * C);
  h2d(ctx, dsh, share, 32 * C);
  h2d(ctx, drn, randomness, 32 * C);
  const uint8_t* dq = upload_mask(ctx, "c3_qualified", qualified, n);
  const uint8_t* df3 = upload_mask(ctx, "c3_fetched3", fetched3, n);
  uint32_t* sr = buf<uint32_t>(ctx, "c3_sr", 32 * 2 * C);
  uint32_t* acc2 = buf<uint32_t>(ctx, "c3_acc2", 4 * 2 * C);
  uint32_t* acd2 = buf<uint32_t>(ctx, "c3_acd2", 4 * 2 * C);
  dkgk::c3_prep(C, n, dacc, dacd, dsh, drn, sr, acc2, acd2, st);
  // P^E_i(j), P^A_i(j): items 2c, 2c + 1 on rows i, n + i.  Both rows of a dealer carry the same item
  // count, so the automatic switch sends them the same way
  std::vector<uint32_t> index(2 * C), row(2 * C);
  for (size_t c = 0; c < C; c++) {
    index[2 * c] = index[2 * c + 1] = accuser[c];
    row[2 * c] = accused[c];
    row[2 * c + 1] = (uint32_t)n + accused[c];
  }
  ComplaintEvals ev;
  complaint_evals(ctx, n, t, 2 * n, 2 * C, index.data(), row.data(), acc2, acd2, EA, EAext, ev);
  uint8_t* eq = buf<uint8_t>(ctx, "c3_eq", 2 * C);
  dkgk::c3_check(C, dacc, sr, ev.dridx, ev.Rh, ev.Rt, ev.scale, ctx->tab_gw, ctx->tab_hw, eq, st);
  int32_t* dver = buf<int32_t>(ctx, "c3_verdict", 4 * C);
  dkgk::c3_final(C, n, dacd, dacd, rowok, dq, df3, eq, dver, st);  // commitment row = dealer row = accused
  check_launch(ctx);
  d2h(ctx, verdict, dver, 4 * C);
  sync(ctx);  // the staging vectors (ev) live until here
}

// proven[i] = some complaint against i holds: verdict 0, or the accused has no phase-3 broadcast
// (committee.rs:643, :664-669)
std::vector<uint8_t> proven_round4(size_t n, size_t C, const uint32_t* accused, const int32_t* verdict) {
  std::vector<uint8_t> p(n, 0);
  for (size_t c = 0; c < C; c++)
    if (verdict[c] == 0 || verdict[c] == DKG_COMPLAINT_NO_PHASE3) p[accused[c] - 1] = 1;
  return p;
}

// The broadcast complaints of a ceremony to verify, as the host arrays of the C ABI (with C = 0 the
// arrays may be null).  Round 2 (dkg_complaints_verify, on the ceremony's own ciphertexts): pk the
// members' keys; verdict [C] out, dissent [n] out (may be null).  Round 4 (dkg_complaints3_verify):
// verdict [C] out, finalise_status / recovery_index out (may be null).
struct Complaints2 {
  const uint8_t* pk;
  size_t C;
  const uint32_t *accuser, *accused;
  const uint8_t* proofs;
  int32_t *verdict, *dissent;
};
struct Complaints4 {
  size_t C;
  const uint32_t *accuser, *accused;
  const uint8_t *share, *randomness;
  int32_t *verdict, *finalise_status, *recovery_index;
};

// What follows a ceremony that took `reconstruct` from the proven round-4 complaints: the verdicts
// against dealers that round 2 disqualified become IGNORED (committee.rs:639), and the finalising
// parties' common outcome.  a_ok[i] = dealer i has a usable phase-3 broadcast.  A qualified dealer
// without one that nobody complained about is in no set: every party's finalise reaches the expect
// at committee.rs:791-795 with indexed_committed_shares[i] never stored (:527-530).  Dealers are
// visited in index order and the first failure wins (:745-797); mpk is zeroed on a panic.
// The finalising parties' common outcome of one ceremony from its sets [n]: the DKG_FIN_* status
// and, in *index, the dealer of INSUFFICIENT / PANIC (else -1).
int32_t finalise_outcome(size_t n, size_t t, const uint8_t* qualified, const uint8_t* recon, const uint8_t* r2_error,
                         const uint8_t* r4_error, const uint8_t* a_ok, bool phase4_error, int32_t* index) {
  *index = -1;
  if (phase4_error) return DKG_FIN_PHASE4_ERROR;
  const bool insufficient = recovery_fails(disclosing_parties(n, qualified, recon, r2_error, r4_error), t);
  for (size_t i = 0; i < n; i++) {
    int32_t status = DKG_FIN_OK;
    if (recon[i] && insufficient) status = DKG_FIN_INSUFFICIENT;
    else if (!recon[i] && qualified[i] && !a_ok[i]) status = DKG_FIN_PANIC;
    if (status != DKG_FIN_OK) {
      *index = (int32_t)i;
      return status;
    }
  }
  return DKG_FIN_OK;
}

void proven_outcome(size_t n, size_t t, const Complaints4& c4, const uint8_t* a_ok, const RoundsResult& r,
                    uint8_t* mpk) {
  const uint8_t *qualified = r.qualified.data(), *recon = r.reconstruct.data();
  for (size_t c = 0; c < c4.C; c++)
    if (!qualified[c4.accused[c] - 1]) c4.verdict[c] = DKG_COMPLAINT_IGNORED;
  int32_t index = -1;
  const int32_t status =
      finalise_outcome(n, t, qualified, recon, r.r2_error.data(), r.r4_error.data(), a_ok, r.phase4_error, &index);
  if (status == DKG_FIN_PANIC) memset(mpk, 0, 32);
  if (c4.finalise_status) *c4.finalise_status = status;
  if (c4.recovery_index) *c4.recovery_index = index;
}

// ---- the proven-complaint rule for batches of ceremonies: the complaint stage on the device
// The broadcast complaints of a whole batch as the flat host arrays of the C ABI: complaint c belongs
// to ceremony[c] (0-based), accuser / accused are 1-based within it; any order, duplicates allowed.
struct BatchComplaints2 {
  const uint8_t* pk;  // [B][n][32]
  size_t C;
  const uint32_t *ceremony, *accuser, *accused;
  const uint8_t* proofs;
  int32_t *verdict, *dissent;  // [C], [B][n] (may be null)
};
struct BatchComplaints4 {
  size_t C;
  const uint32_t *ceremony, *accuser, *accused;
  const uint8_t *share, *randomness;
  int32_t *verdict, *finalise_status, *recovery_index;  // [C], [B], [B] (the last two may be null)
};

bool batch_complaint_args_ok(size_t B, size_t n, size_t C, const uint32_t* ceremony, const uint32_t* accuser,
                             const uint32_t* accused, std::initializer_list<const void*> payload) {
  if (!C) return true;
  if (!ceremony) return false;
  for (size_t c = 0; c < C; c++)
    if (ceremony[c] >= B) return false;
  return complaint_args_ok(n, C, accuser, accused, payload);
}

// The per-complaint index arrays of one round's complaints (host, O(C)): the evaluation index x =
// accuser, the party row g n + accuser, the 1-based dealer row g n + accused, and the commitment row
// = the accused's place (1-based) among the DISTINCT accused dealer rows `rows` (0-based), which are
// all the stage decodes.
struct ComplaintIndex {
  std::vector<uint32_t> party, drow, crow, rows;
};
ComplaintIndex complaint_index(size_t n, size_t C, const uint32_t* ceremony, const uint32_t* accuser,
                               const uint32_t* accused) {
  ComplaintIndex ix;
  ix.party.resize(C), ix.drow.resize(C), ix.crow.resize(C);
  std::unordered_map<uint32_t, uint32_t> place;
  for (size_t c = 0; c < C; c++) {
    const uint32_t base = ceremony[c] * (uint32_t)n;
    ix.party[c] = base + accuser[c];
    ix.drow[c] = base + accused[c];
    auto it = place.find(ix.drow[c]);
    if (it == place.end()) {
      ix.rows.push_back(ix.drow[c] - 1);
      it = place.emplace(ix.drow[c], (uint32_t)ix.rows.size()).first;
    }
    ix.crow[c] = it->second;
  }
  return ix;
}

// What verify_batch has put on the device of a BatchInput (null = absent): E, A [V][N][8]; plaintext
// shares s, s_prime [V][n][8] or, in full mode, sk [V][8] and e1, ct [V][n][2][8]; the masks [V].
struct BatchDevice {
  const uint32_t *E = nullptr, *A = nullptr;
  const uint32_t *s = nullptr, *s_prime = nullptr;
  const uint32_t *sk = nullptr, *e1 = nullptr, *ct = nullptr;
  const uint8_t *fetched1 = nullptr, *fetched3 = nullptr;
};

// The two complaint stages on GATHERED rows, shared by a batch (batch_complaints gathers on the device from
// its own uploads) and by the hosted operator's calls (complaints_ceremonies gathers on the host): queued
// on ctx->stream, no synchronisation, a launch count that depends on nothing.  Always the per-complaint
// Horner walk (k_cmp_horner).  Device index arrays [C] as ComplaintIndex names them, seq = 0, 1, 2, ..
// Round 4 (k_c3_*): rc [2 R][N][8] the accused dealers' E rows, then their A rows; share / randomness
// host [C][32]; qualified / fetched3 (device, may be null) by dealer row drow; dver [C] out.
void complaints4_rows(dkg_ctx* ctx, size_t n, size_t t, size_t C4, size_t R4, const uint32_t* rc, const uint32_t* x4,
                      const uint32_t* crow4, const uint32_t* drow4, const uint32_t* seq, const uint8_t* share,
                      const uint8_t* randomness, const uint8_t* qualified, const uint8_t* fetched3, int32_t* dver4) {
  const size_t N = t + 1;
  hipStream_t st = ctx->stream;
  int nb = 1;
  while ((n >> nb) != 0) nb++;
  uint32_t* rext = buf<uint32_t>(ctx, "bp.rows4_ext", PTB * 2 * R4 * N);
  uint8_t* pok = buf<uint8_t>(ctx, "bp.rows4_pok", 2 * R4 * N);
  uint8_t* rowok = buf<uint8_t>(ctx, "bp.rows4_ok", 2 * R4);
  dkgk::decode_points(rc, 2 * R4 * N, rext, 2 * R4 * N, pok, st);
  dkgk::dealer_ok(2 * R4, N, pok, rowok, st);
  uint32_t* dsh = buf<uint32_t>(ctx, "bp.share", 32 * C4);
  uint32_t* drn = buf<uint32_t>(ctx, "bp.rand", 32 * C4);
  h2d(ctx, dsh, share, 32 * C4);
  h2d(ctx, drn, randomness, 32 * C4);
  uint32_t* sr = buf<uint32_t>(ctx, "bp.sr", 32 * 2 * C4);
  uint32_t* acc2 = buf<uint32_t>(ctx, "bp.acc2", 4 * 2 * C4);
  uint32_t* acd2 = buf<uint32_t>(ctx, "bp.acd2", 4 * 2 * C4);
  dkgk::c3_prep(C4, R4, x4, crow4, dsh, drn, sr, acc2, acd2, st);
  uint32_t* Rh = buf<uint32_t>(ctx, "bp.Rh4", PTB * 2 * C4);
  dkgk::cmp_horner(2 * C4, seq, acc2, acd2, rext, 2 * R4 * N, N, nb, Rh, st);
  uint8_t* eq = buf<uint8_t>(ctx, "bp.eq4", 2 * C4);
  dkgk::c3_check(C4, x4, sr, seq, Rh, nullptr, nullptr, ctx->tab_gw, ctx->tab_hw, eq, st);
  dkgk::c3_final(C4, R4, crow4, drow4, rowok, qualified, fetched3, eq, dver4, st);
}
// Round 2 (k_cv_*): rc [R][N][8] the accused dealers' E rows; dpk the stacked member keys, party2 the
// accusers' 1-based rows of it; denc [C][128] (device) the pairs the accused sent; proofs host [C][192];
// fetched (device, may be null) [R] by the commitment row's place; dver [C] out.
void complaints2_rows(dkg_ctx* ctx, size_t n, size_t t, size_t C2, size_t R2, const uint32_t* rc, const uint32_t* x2,
                      const uint32_t* party2, const uint32_t* crow2, const uint32_t* seq, const uint32_t* dpk,
                      const uint32_t* denc, const uint8_t* proofs, const uint8_t* fetched, int32_t* dver2) {
  const size_t N = t + 1;
  hipStream_t st = ctx->stream;
  int nb = 1;
  while ((n >> nb) != 0) nb++;
  uint32_t* rext = buf<uint32_t>(ctx, "bp.rows2_ext", PTB * R2 * N);
  uint8_t* pok = buf<uint8_t>(ctx, "bp.rows2_pok", R2 * N);
  uint8_t* rowok = buf<uint8_t>(ctx, "bp.rows2_ok", R2);
  dkgk::decode_points(rc, R2 * N, rext, R2 * N, pok, st);
  dkgk::dealer_ok(R2, N, pok, rowok, st);
  uint32_t* dprf = buf<uint32_t>(ctx, "bp.proofs", 192 * C2);
  h2d(ctx, dprf, proofs, 192 * C2);
  // the party rows stand where one ceremony has the accusers, the commitment rows where it has the accused
  const Announcements an = complaint_announcements(ctx, C2, party2, dpk, denc, dprf, st);
  uint32_t* Rh = buf<uint32_t>(ctx, "bp.Rh2", PTB * C2);
  dkgk::cmp_horner(C2, seq, x2, crow2, rext, R2 * N, N, nb, Rh, st);
  uint8_t* eq = buf<uint8_t>(ctx, "bp.eq2", 2 * C2);
  dkgk::cv_check(C2, x2, an.p12, seq, Rh, nullptr, nullptr, ctx->tab_gw, ctx->tab_hw, eq, st);
  dkgk::cv_final(C2, party2, crow2, dpk, denc, dprf, an.a1c, an.a2c, an.ppok, rowok, fetched, eq, dver2, st);
}

// Both complaint stages of a batch, queued on ctx->stream after the batch's uploads and before its
// rounds; no host synchronisation, host work O(C), a launch count that does not depend on B and no
// copy per row, ceremony or complaint.  Round 4 first, as verify_ceremony.  c2 comes with full mode
// only (dev.e1, dev.ct).  Always the per-complaint Horner walk (k_cmp_horner): ctx->complaint_eval
// does not apply.  Leaves the masks and the device verdicts in bp; the index arrays go through one
// pinned staging buffer.
enum { BP_C4, BP_C2 };
const PhaseRow BPROVEN_PHASES[] = {{"c4", 1u << BP_C4}, {"c2", 1u << BP_C2}};
void batch_complaints(dkg_ctx* ctx, size_t B, size_t n, size_t t, const BatchDevice& dev, const BatchComplaints2* c2,
                      const BatchComplaints4& c4, BatchProven& bp) {
  const size_t N = t + 1, V = B * n, C2 = c2 ? c2->C : 0, C4 = c4.C;
  hipStream_t st = ctx->stream;
  const ComplaintIndex i4 = complaint_index(n, C4, c4.ceremony, c4.accuser, c4.accused);
  const ComplaintIndex i2 = c2 ? complaint_index(n, C2, c2->ceremony, c2->accuser, c2->accused) : ComplaintIndex{};
  const size_t R4 = i4.rows.size(), R2 = i2.rows.size(), iota = std::max(2 * C4, C2);
  // one upload: x4 | crow4 | drow4 | rows4 | x2 | party2 | crow2 | drow2 | rows2 | 0, 1, 2, ..
  const size_t words = 3 * C4 + R4 + 4 * C2 + R2 + iota;
  uint32_t* hix = hbuf<uint32_t>(ctx, "hb.bp_idx", 4 * words);
  uint32_t* dix = buf<uint32_t>(ctx, "bp.idx", 4 * words);
  size_t at = 0;
  auto put = [&](const uint32_t* src, size_t cnt) {
    const uint32_t* d = dix + at;
    if (cnt) memcpy(hix + at, src, 4 * cnt);
    at += cnt;
    return d;
  };
  const uint32_t* x4 = put(c4.accuser, C4);
  const uint32_t* crow4 = put(i4.crow.data(), C4);
  const uint32_t* drow4 = put(i4.drow.data(), C4);
  const uint32_t* rows4 = put(i4.rows.data(), R4);
  const uint32_t* x2 = put(c2 ? c2->accuser : nullptr, C2);
  const uint32_t* party2 = put(i2.party.data(), C2);
  const uint32_t* crow2 = put(i2.crow.data(), C2);
  const uint32_t* drow2 = put(i2.drow.data(), C2);
  const uint32_t* rows2 = put(i2.rows.data(), R2);
  const uint32_t* seq = dix + at;  // list and ridx of the Horner walks: item k is element k of Rh
  for (size_t k = 0; k < iota; k++) hix[at + k] = (uint32_t)k;
  h2d(ctx, dix, hix, 4 * words);
  phase_mark(ctx, st, "bproven", -1);
  // ---- round 4 (k_c3_*): the E and A rows of the accused dealers, gathered and decoded once
  uint8_t* proven4 = buf<uint8_t>(ctx, "bp.proven4", V);
  int32_t* dver4 = buf<int32_t>(ctx, "bp.verdict4", 4 * C4);
  HCK(hipMemsetAsync(proven4, 0, V, st));
  if (C4) {
    uint32_t* rc = buf<uint32_t>(ctx, "bp.rows4", 32 * 2 * R4 * N);
    dkgk::gather_rows(R4, N, rows4, dev.E, dev.A, rc, st);
    // the qualified set is applied on the host (IGNORED, batch_proven_outcome), as verify_ceremony does
    complaints4_rows(ctx, n, t, C4, R4, rc, x4, crow4, drow4, seq, c4.share, c4.randomness, nullptr, dev.fetched3,
                     dver4);
  }
  phase_mark(ctx, st, "bproven", BP_C4);
  // ---- round 2 (k_cv_*): the E rows of the accused dealers, the ciphertext pairs from the batch's own
  uint8_t *cmask = nullptr, *pair = nullptr;
  int32_t* dver2 = nullptr;
  if (c2) {
    cmask = buf<uint8_t>(ctx, "bp.cmask", V);
    pair = buf<uint8_t>(ctx, "bp.pair", V * n);
    dver2 = buf<int32_t>(ctx, "bp.verdict2", 4 * C2);
    HCK(hipMemsetAsync(cmask, 1, V, st));
    HCK(hipMemsetAsync(pair, 0, V * n, st));
  }
  if (C2) {
    uint32_t* rc = buf<uint32_t>(ctx, "bp.rows2", 32 * R2 * N);
    dkgk::gather_rows(R2, N, rows2, dev.E, nullptr, rc, st);
    uint32_t* dpk = buf<uint32_t>(ctx, "bp.pk", 32 * V);
    uint32_t* denc = buf<uint32_t>(ctx, "bp.enc", 128 * C2);
    h2d(ctx, dpk, c2->pk, 32 * V);
    dkgk::gather_enc(C2, n, drow2, x2, dev.e1, dev.ct, denc, st);
    complaints2_rows(ctx, n, t, C2, R2, rc, x2, party2, crow2, seq, dpk, denc, c2->proofs, nullptr, dver2);
  }
  // ---- the verdicts as the rounds' masks
  dkgk::proven_masks(C2, n, drow2, x2, dver2, C4, drow4, dver4, cmask, pair, proven4, st);
  if (c2) phase_mark(ctx, st, "bproven", BP_C2);  // without a round-2 stage bproven.c2 reads -1
  check_launch(ctx);
  bp.a_ok = dev.fetched3;
  bp.cmask = cmask;
  bp.pair = pair;
  bp.proven4 = proven4;
  bp.dver2 = dver2;
  bp.dver4 = dver4;
  bp.C2 = C2;
  bp.C4 = C4;
  bp.verdict2 = c2 ? c2->verdict : nullptr;
  bp.dissent = c2 ? c2->dissent : nullptr;
  bp.verdict4 = c4.verdict;
}

// After the batch's sync: the stages' device times, and per ceremony what proven_outcome does for one --
// the verdicts against dealers that round 2 disqualified become IGNORED, the finalising parties' common
// outcome, and a zeroed mpk where they panic.
void batch_proven_outcome(dkg_ctx* ctx, size_t B, size_t n, size_t t, const BatchComplaints4& c4,
                          const BatchProven& bp, dkg_batch_out* out) {
  phase_collect(ctx, "bproven", BPROVEN_PHASES, std::size(BPROVEN_PHASES));
  for (size_t c = 0; c < c4.C; c++)
    if (!bp.qualified[(size_t)c4.ceremony[c] * n + c4.accused[c] - 1]) c4.verdict[c] = DKG_COMPLAINT_IGNORED;
  for (size_t g = 0; g < B; g++) {
    const size_t o = g * n;
    int32_t index = -1;
    const int32_t status = finalise_outcome(n, t, &bp.qualified[o], &bp.reconstruct[o], &bp.r2_error[o], &bp.r4_error[o],
                                            &bp.a_present[o], bp.phase4_error[g] != 0, &index);
    if (status == DKG_FIN_PANIC && out->mpk) memset(out->mpk + 32 * g, 0, 32);
    if (c4.finalise_status) c4.finalise_status[g] = status;
    if (c4.recovery_index) c4.recovery_index[g] = index;
  }
}

// One ceremony to verify, as the host pointers of the C ABI (null = absent).  The shares come either
// in plaintext (s, s_prime) or encrypted with the members' keys (e1, ct, sk: full mode).  c2 / c4
// decide whether a round's outcome follows the PROVEN complaints instead of the receivers' own
// rejections -- their presence does, not C > 0: no complaints under the proven rule disqualify nobody.
struct CeremonyInput {
  const uint8_t *E = nullptr, *A = nullptr;                         // required
  const uint8_t *s = nullptr, *s_prime = nullptr;                   // plaintext shares, or
  const uint8_t *e1 = nullptr, *ct = nullptr, *sk = nullptr;        //   encrypted shares and the members' keys
  const uint8_t *fetched1 = nullptr, *fetched3 = nullptr;           // intake masks
  const Complaints2* c2 = nullptr;
  const Complaints4* c4 = nullptr;
};

// Rounds 2-5 of a ceremony from its broadcast values: every dkg_ceremony_verify* entry point.  The
// commitments go to the device once, for both complaint cores and the rounds; the complaints are
// verified before the timed region (ev[0]), which covers the decryption and the rounds as ms_* report.
int verify_ceremony(dkg_ctx* ctx, size_t n, size_t t, const CeremonyInput& in, dkg_ceremony_out* out) {
  const size_t N = t + 1, items = 2 * n * n;
  const bool full = in.e1 != nullptr;
  const Commitments cm = upload_commitments(ctx, n, N, in.E, in.A);
  RoundMasks m;
  // the round-4 complaints first: their verdicts do not depend on the qualified set, only whether
  // they count (proven_outcome).  a_ok[i] = dealer i has a usable phase-3 broadcast
  std::vector<uint8_t> proven, a_ok(n);
  if (in.c4) {
    const Complaints4& c = *in.c4;
    std::vector<uint8_t> rowok(2 * n);
    complaints3_core(ctx, n, t, c.C, c.accuser, c.accused, c.share, c.randomness, cm.E, nullptr, in.fetched3,
                     c.verdict, rowok.data());
    proven = proven_round4(n, c.C, c.accused, c.verdict);
    uint8_t* dp4 = buf<uint8_t>(ctx, "c3_proven", n);
    h2d(ctx, dp4, proven.data(), n);
    m.proven4 = dp4;
    for (size_t i = 0; i < n; i++) a_ok[i] = (!in.fetched3 || in.fetched3[i]) && rowok[n + i];
  }
  m.e_ok = upload_mask(ctx, "cer_f1", in.fetched1, n);
  m.a_ok = upload_mask(ctx, "cer_f3", in.fetched3, n);
  std::vector<uint8_t> enc, cmask;
  if (in.c2) {
    const Complaints2& c = *in.c2;
    // the complaints against this ceremony's own broadcasts: the pair the accused sent the accuser
    // (broadcast.rs:57), items (i, q, w) at (i n + q) 2 + w, w = 0 the randomness
    enc.resize(128 * c.C);
    for (size_t k = 0; k < c.C; k++) {
      const size_t item = ((size_t)(c.accused[k] - 1) * n + (c.accuser[k] - 1)) * 2;
      const uint8_t* part[4] = {in.e1 + 32 * item, in.ct + 32 * item, in.e1 + 32 * (item + 1),
                                in.ct + 32 * (item + 1)};
      for (size_t p = 0; p < 4; p++) memcpy(&enc[128 * k + 32 * p], part[p], 32);
    }
    uint32_t* dpk = buf<uint32_t>(ctx, "cv_pk", 32 * n);
    h2d(ctx, dpk, c.pk, 32 * n);
    complaints_verify_core(ctx, n, t, c.C, c.accuser, c.accused, dpk, cm.E, nullptr, enc.data(), c.proofs, c.verdict,
                           nullptr);
    cmask.assign(n, 1);  // the dealers without a proven complaint (committee.rs:381-394: cleared only on Ok)
    for (size_t k = 0; k < c.C; k++)
      if (c.verdict[k] == 0) cmask[c.accused[k] - 1] = 0;
    uint8_t* dcm = buf<uint8_t>(ctx, "cv_cmask", n);
    h2d(ctx, dcm, cmask.data(), n);
    m.cmask = dcm;
    sync(ctx);
  }
  const uint32_t *ds = nullptr, *dsp = nullptr, *dsk = nullptr;
  uint32_t *de1 = nullptr, *dct = nullptr;
  if (full) {
    dsk = upload_scalars(ctx, "fm_sk", in.sk, n);
    de1 = buf<uint32_t>(ctx, "fm_e1", 32 * items);
    dct = buf<uint32_t>(ctx, "fm_ct", 32 * items);
    h2d(ctx, de1, in.e1, 32 * items);
    h2d(ctx, dct, in.ct, 32 * items);
  } else {
    ds = upload_scalars(ctx, "cer_s", in.s, n * n);
    dsp = upload_scalars(ctx, "cer_sp", in.s_prime, n * n);
  }
  HCK(hipEventRecord(ctx->ev[0], ctx->stream));
  HCK(hipEventRecord(ctx->ev[1], ctx->stream));
  if (full) {
    uint32_t* rs = buf<uint32_t>(ctx, "fm_s", 32 * n * n);
    uint32_t* rsp = buf<uint32_t>(ctx, "fm_sp", 32 * n * n);
    uint8_t* iok = buf<uint8_t>(ctx, "fm_iok", items);
    uint8_t* eok = buf<uint8_t>(ctx, "fm_eok", n);
    // the decryption on the side stream beside the check pipeline, as in dkg_ceremony_run_full_device
    const bool side = ctx->nsub > 1 && ctx->verify_mode == 0;
    if (side) {
      HCK(hipEventRecord(ctx->side_fork, ctx->stream));
      HCK(hipStreamWaitEvent(ctx->side, ctx->side_fork, 0));
    }
    decrypt_device(ctx, n, n, dsk, de1, dct, rs, rsp, iok, eok, side ? ctx->side : ctx->stream);
    if (side) {
      HCK(hipEventRecord(ctx->shares_done, ctx->side));
      ctx->shares_pending = true;
    }
    ds = rs, dsp = rsp;
    m.e_ok = eok;  // the decode mask of the dealer's ciphertexts
  }
  const RoundsResult r = receivers_rounds(ctx, n, t, cm.E, cm.A, ds, dsp, out, true, m);  // waits for the shares
  if (full) {
    phase_collect(ctx, "full", FULL_PHASES, std::size(FULL_PHASES));  // no encryption here: full.enc_* read -1
    if (out->s) d2h(ctx, out->s, ds, 32 * n * n);
    if (out->s_prime) d2h(ctx, out->s_prime, dsp, 32 * n * n);
    sync(ctx);
  }
  ceremony_times(ctx, out, false);
  if (in.c4) proven_outcome(n, t, *in.c4, a_ok.data(), r, out->mpk);
  if (in.c2 && in.c2->dissent)
    complaint_dissent(ctx, n, in.c2->C, in.c2->accuser, in.c2->accused, in.c2->verdict, in.c2->dissent);
  return DKG_OK;
}

// B stacked ceremonies to verify, as the host pointers of the C ABI (null = absent), in the manner of
// CeremonyInput: plaintext shares (s, s_prime) or full mode (e1, ct, sk); the presence of c4 selects
// the proven rule, c2 comes with full mode only.  s_out / s_prime_out receive the decrypted shares.
struct BatchInput {
  const uint8_t *E = nullptr, *A = nullptr;                   // required
  const uint8_t *s = nullptr, *s_prime = nullptr;             // plaintext shares, or
  const uint8_t *e1 = nullptr, *ct = nullptr, *sk = nullptr;  //   encrypted shares and the members' keys
  const uint8_t *fetched1 = nullptr, *fetched3 = nullptr;     // intake masks
  const BatchComplaints2* c2 = nullptr;
  const BatchComplaints4* c4 = nullptr;
  uint8_t *s_out = nullptr, *s_prime_out = nullptr;
};

// Rounds 2-5 of a batch from its broadcast values: every dkg_ceremony_batch_verify* entry point.  The
// complaint stage is queued before the timed region (ev[0]), which covers the decryption and the
// rounds as ms_* report.
int verify_batch(dkg_ctx* ctx, size_t B, size_t n, size_t t, const BatchInput& in, dkg_batch_out* out) {
  const size_t N = t + 1, V = B * n, items = 2 * V * n;
  const bool full = in.e1 != nullptr;
  BatchDevice d;
  uint32_t* Ec = buf<uint32_t>(ctx, "bat_E", 32 * V * N);
  uint32_t* Ac = buf<uint32_t>(ctx, "bat_A", 32 * V * N);
  h2d(ctx, Ec, in.E, 32 * V * N);
  h2d(ctx, Ac, in.A, 32 * V * N);
  d.E = Ec, d.A = Ac;
  if (full) {
    d.sk = upload_scalars(ctx, "bfm_sk", in.sk, V);
    uint32_t* de1 = buf<uint32_t>(ctx, "bfm_e1", 32 * items);
    uint32_t* dct = buf<uint32_t>(ctx, "bfm_ct", 32 * items);
    h2d(ctx, de1, in.e1, 32 * items);
    h2d(ctx, dct, in.ct, 32 * items);
    d.e1 = de1, d.ct = dct;
  } else {
    d.s = upload_scalars(ctx, "bat_s", in.s, V * n);
    d.s_prime = upload_scalars(ctx, "bat_sp", in.s_prime, V * n);
  }
  d.fetched1 = upload_mask(ctx, "bp.f1", in.fetched1, V);
  d.fetched3 = upload_mask(ctx, "bp.f3", in.fetched3, V);
  BatchProven bp;
  if (in.c4) batch_complaints(ctx, B, n, t, d, full ? in.c2 : nullptr, *in.c4, bp);
  HCK(hipEventRecord(ctx->ev[0], ctx->stream));
  HCK(hipEventRecord(ctx->ev[1], ctx->stream));
  const uint8_t* e_ok = d.fetched1;
  if (full) {
    uint32_t* rs = buf<uint32_t>(ctx, "bfm_s", 32 * V * n);
    uint32_t* rsp = buf<uint32_t>(ctx, "bfm_sp", 32 * V * n);
    uint8_t* iok = buf<uint8_t>(ctx, "bfm_iok", items);
    uint8_t* eok = buf<uint8_t>(ctx, "bfm_eok", V);
    decrypt_batch_device(ctx, B, n, d.sk, d.e1, d.ct, rs, rsp, iok, eok);
    d.s = rs, d.s_prime = rsp;
    e_ok = eok;  // the decode mask of the dealer's ciphertexts
  }
  batch_receivers(ctx, B, n, t, d.E, d.A, d.s, d.s_prime, out, e_ok, in.c4 ? &bp : nullptr);
  if (full) phase_collect(ctx, "bfull", BF_ROWS, BF_PHASES);
  if (in.c4) batch_proven_outcome(ctx, B, n, t, *in.c4, bp, out);
  if (full) {
    if (in.s_out) d2h(ctx, in.s_out, d.s, 32 * V * n);
    if (in.s_prime_out) d2h(ctx, in.s_prime_out, d.s_prime, 32 * V * n);
    sync(ctx);
  }
  batch_times(ctx, out, false);
  return DKG_OK;
}

// DKG_E_DECODE when a recipient key of the last encrypt_batch_device did not decode (after a sync)
int batch_keys_status(dkg_ctx* ctx, const uint8_t* ok, size_t V) {
  for (size_t k = 0; k < V; k++)
    if (!ok[k]) {
      ctx->err = "encrypt_shares_batch: a recipient public key does not decode";
      return DKG_E_DECODE;
    }
  return DKG_OK;
}

}  // namespace

// dkg_ctx_clock_probe: a dependent integer chain per lane between two reads of each clock; lane 0
// of every wave writes (shader cycles, constant-clock ticks) with vector stores.
__global__ __launch_bounds__(256) void k_clock_probe(unsigned iters, unsigned long long* out) {
  uint32_t x = threadIdx.x * 2654435761u + blockIdx.x;
  const unsigned long long c0 = clock64(), r0 = wall_clock64();
  for (unsigned i = 0; i < iters; i++) x = x * 1664525u + 1013904223u;
  asm volatile("" : "+v"(x));
  const unsigned long long c1 = clock64(), r1 = wall_clock64();
  const size_t w = (size_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
  if ((threadIdx.x & 63) == 0) {
    out[2 * w] = (c1 - c0) + (x == 0xffffffffu ? 1 : 0);  // x kept live: the chain is not dead code
    out[2 * w + 1] = r1 - r0;
  }
}

extern "C" {

int dkg_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int dkg_device_pci_bus_id(int device, char* buf, int len) {
  if (!buf || len < 13) return DKG_E_ARG;
  return hipDeviceGetPCIBusId(buf, len, device) == hipSuccess ? DKG_OK : DKG_E_DEVICE;
}

int dkg_ctx_clock_probe(dkg_ctx* ctx, unsigned iters, double* sclk_mhz, double* busy_ms) {
  return guarded(ctx, [&] {
    if (!sclk_mhz || !busy_ms || !iters) return DKG_E_ARG;
    int cus = 0, wall_khz = 0;
    HCK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    HCK(hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, ctx->device));
    if (cus <= 0 || wall_khz <= 0) return DKG_E_DEVICE;
    const size_t waves = (size_t)cus * 16;  // 4 workgroups of 4 waves per CU: 4 waves per SIMD
    unsigned long long* d = buf<unsigned long long>(ctx, "clock_probe", 2 * 8 * waves);
    hipLaunchKernelGGL(k_clock_probe, dim3((unsigned)(waves / 4)), dim3(256), 0, ctx->stream, iters, d);
    check_launch(ctx);
    std::vector<unsigned long long> h(2 * waves);
    d2h(ctx, h.data(), d, 2 * 8 * waves);
    sync(ctx);
    std::vector<double> mhz(waves), ms(waves);
    for (size_t w = 0; w < waves; w++) {
      const double real_us = (double)h[2 * w + 1] / wall_khz * 1e3;
      mhz[w] = real_us > 0 ? (double)h[2 * w] / real_us : 0.0;
      ms[w] = real_us / 1e3;
    }
    std::nth_element(mhz.begin(), mhz.begin() + waves / 2, mhz.end());
    std::nth_element(ms.begin(), ms.begin() + waves / 2, ms.end());
    *sclk_mhz = mhz[waves / 2];
    *busy_ms = ms[waves / 2];
    return DKG_OK;
  });
}

int dkg_ctx_create(int device, dkg_ctx** out) {
  if (!out) return DKG_E_ARG;
  *out = nullptr;
  dkg_ctx* ctx = new dkg_ctx();
  ctx->device = device;
  int rc = guarded(ctx, [&] {
    // the ceremony's own streams at the highest priority, the side stream at the lowest: a
    // latency-bound binomial step must not queue behind the side stream's share evaluation
    int least = 0, greatest = 0;
    HCK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    HCK(hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, greatest));
    for (auto& e : ctx->ev) HCK(hipEventCreate(&e));
    ctx->phase_pool.resize(PHASE_POOL_MIN);
    for (auto& e : ctx->phase_pool) HCK(hipEventCreate(&e));
    for (auto& e : ctx->cb_ev) HCK(hipEventCreate(&e));
    for (auto& st : ctx->sub) HCK(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, greatest));
    HCK(hipStreamCreateWithPriority(&ctx->side, hipStreamNonBlocking, least));
    HCK(hipEventCreateWithFlags(&ctx->side_fork, hipEventDisableTiming));
    HCK(hipEventCreateWithFlags(&ctx->shares_done, hipEventDisableTiming));
    HCK(hipEventCreateWithFlags(&ctx->pub_done, hipEventDisableTiming));
    HCK(hipEventCreateWithFlags(&ctx->terms_done, hipEventDisableTiming));
    HCK(hipEventCreateWithFlags(&ctx->fork, hipEventDisableTiming));
    for (auto& e : ctx->join) HCK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HCK(hipMalloc(&ctx->tab_g, COMB_BYTES));
    HCK(hipMalloc(&ctx->tab_h, COMB_BYTES));
    HCK(hipMalloc(&ctx->tab_gw, COMBW_BYTES));
    HCK(hipMalloc(&ctx->tab_hw, COMBW_BYTES));
    bool ok = false;
    comb_for_point(ctx, BASEPOINT, ctx->tab_g, &ok, ctx->tab_gw);
    if (!ok) {
      ctx->err = "basepoint failed to decode on device";
      return DKG_E_DEVICE;
    }
    return DKG_OK;
  });
  if (rc != DKG_OK) {
    fprintf(stderr, "dkg_ctx_create: %s\n", ctx->err.c_str());
    dkg_ctx_destroy(ctx);
    return rc;
  }
  *out = ctx;
  return DKG_OK;
}

void dkg_ctx_destroy(dkg_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipDeviceSynchronize();
  for (auto& kv : ctx->bufs) (void)hipFree(kv.second.first);
  for (auto& kv : ctx->hbufs) (void)hipHostFree(kv.second.first);
  if (ctx->tab_g) (void)hipFree(ctx->tab_g);
  if (ctx->tab_h) (void)hipFree(ctx->tab_h);
  if (ctx->tab_gw) (void)hipFree(ctx->tab_gw);
  if (ctx->tab_hw) (void)hipFree(ctx->tab_hw);
  for (auto& e : ctx->ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : ctx->phase_pool)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : ctx->cb_ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : ctx->join)
    if (e) (void)hipEventDestroy(e);
  if (ctx->fork) (void)hipEventDestroy(ctx->fork);
  for (auto& st : ctx->sub)
    if (st) (void)hipStreamDestroy(st);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  if (ctx->side) (void)hipStreamDestroy(ctx->side);
  if (ctx->side_fork) (void)hipEventDestroy(ctx->side_fork);
  if (ctx->shares_done) (void)hipEventDestroy(ctx->shares_done);
  if (ctx->pub_done) (void)hipEventDestroy(ctx->pub_done);
  if (ctx->terms_done) (void)hipEventDestroy(ctx->terms_done);
  delete ctx;
}

const char* dkg_ctx_last_error(const dkg_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

double dkg_ctx_phase_ms(const dkg_ctx* ctx, const char* name) {
  if (!ctx || !name) return -1.0;
  auto it = ctx->phase_ms.find(name);
  return it == ctx->phase_ms.end() ? -1.0 : it->second;
}

int dkg_ctx_set_streams(dkg_ctx* ctx, int nsub) {
  if (!ctx || nsub < 1 || nsub > dkg_ctx::MAX_SUB) return DKG_E_ARG;
  ctx->nsub = nsub;
  return DKG_OK;
}

int dkg_ctx_set_verify_mode(dkg_ctx* ctx, int mode) {
  if (!ctx || mode < 0 || mode > 1) return DKG_E_ARG;
  ctx->verify_mode = mode;
  return DKG_OK;
}

size_t dkg_ctx_fallback_rows(const dkg_ctx* ctx) { return ctx ? ctx->fallback_rows : 0; }

int dkg_ctx_set_split(dkg_ctx* ctx, int pieces) {
  if (!ctx || pieces < 0 || pieces > 16) return DKG_E_ARG;
  ctx->split = pieces;
  return DKG_OK;
}

int dkg_ctx_set_binomial(dkg_ctx* ctx, int mode) {
  if (!ctx || mode < 0 || mode > 5) return DKG_E_ARG;
  ctx->binom_mode = mode;
  return DKG_OK;
}

int dkg_ctx_set_check(dkg_ctx* ctx, int mode) {
  if (!ctx || mode < 0 || mode > 1) return DKG_E_ARG;
  ctx->check_mode = mode;
  return DKG_OK;
}

int dkg_ctx_set_field_mode(dkg_ctx* ctx, int mode) {
  if (!ctx || mode < 0 || mode > 2) return DKG_E_ARG;
  ctx->fe_mode = mode;
  return DKG_OK;
}

int dkg_ctx_set_stepping(dkg_ctx* ctx, int mode) {
  if (!ctx || mode < 0 || mode > 3) return DKG_E_ARG;
  ctx->step_mode = mode;
  return DKG_OK;
}

int dkg_ctx_last_split(const dkg_ctx* ctx) { return ctx ? ctx->last_split : 0; }
size_t dkg_ctx_last_split_len(const dkg_ctx* ctx) { return ctx ? ctx->last_split_len : 0; }
int dkg_ctx_set_combine(dkg_ctx* ctx, int mode) {
  if (!ctx || mode < 0 || mode > 3) return DKG_E_ARG;
  ctx->combine_mode = mode;
  return DKG_OK;
}
int dkg_ctx_last_combine(const dkg_ctx* ctx) { return ctx ? ctx->last_combine : 0; }
int dkg_ctx_last_binomial(const dkg_ctx* ctx) { return ctx ? ctx->last_binomial : 0; }
int dkg_ctx_set_stepping_formula(dkg_ctx* ctx, int mode) {
  if (!ctx || mode < 0 || mode > 1) return DKG_E_ARG;
  ctx->step_formula = mode;
  return DKG_OK;
}
long long dkg_ctx_stepping_redos(dkg_ctx* ctx) {
  if (!ctx) return -1;
  if (!ctx->last_step_flags) return 0;
  try {
    std::vector<uint32_t> h(ctx->last_step_flag_words);
    sync(ctx);
    HCK(hipMemcpy(h.data(), ctx->last_step_flags, 4 * h.size(), hipMemcpyDeviceToHost));
    long long c = 0;
    for (uint32_t x : h) c += x != 0;
    return c;
  } catch (const Fail& f) {
    return -1;
  }
}
int dkg_ctx_binomial_reruns(dkg_ctx* ctx) { return ctx ? ctx->last_binom_rerun : -1; }
long long dkg_ctx_binomial_wave_redos(dkg_ctx* ctx) {
  if (!ctx) return -1;
  if (!ctx->last_bflags) return 0;
  try {
    std::vector<uint32_t> h(ctx->last_bflag_words);
    sync(ctx);
    HCK(hipMemcpy(h.data(), ctx->last_bflags, 4 * h.size(), hipMemcpyDeviceToHost));
    long long c = 0;
    for (uint32_t x : h) c += x != 0;
    return c;
  } catch (const Fail& f) {
    return -1;
  }
}
int dkg_ctx_set_addends(dkg_ctx* ctx, int mode) {
  if (!ctx || mode < 0 || mode > 1) return DKG_E_ARG;
  ctx->addend_mode = mode;
  return DKG_OK;
}
int dkg_split_multipliers(size_t n, size_t L, int pieces, uint8_t* mag, int8_t* sign) {
  if (!n || !L || pieces < 2 || pieces > (int)SHORT_MAX || !mag || !sign) return DKG_E_ARG;
  try {
    std::vector<uint8_t> m;
    std::vector<int8_t> sg;
    short_vectors(n, L, (size_t)pieces, m, sg, jsf_built((size_t)pieces));  // the default mode's rows
    memcpy(mag, m.data(), m.size());
    memcpy(sign, sg.data(), sg.size());
  } catch (const std::exception&) {
    return DKG_E_NOMEM;
  }
  return DKG_OK;
}
int dkg_jsf_digits(const uint8_t a[32], const uint8_t b[32], int8_t da[256], int8_t db[256], int16_t* top) {
  if (!a || !b || !da || !db || !top) return DKG_E_ARG;
  return dkgh::jsf_digits(a, b, da, db, top) ? DKG_OK : DKG_E_ARG;
}
int dkg_seat_enc_digits(const uint8_t k[32], int8_t digits[128], int* windows) {
  if (!k || !digits || !windows || (k[31] & 0x80)) return DKG_E_ARG;
  uint32_t w[8];
  for (int i = 0; i < 8; i++)
    w[i] = (uint32_t)k[4 * i] | (uint32_t)k[4 * i + 1] << 8 | (uint32_t)k[4 * i + 2] << 16 | (uint32_t)k[4 * i + 3] << 24;
  int carry = 0;
  for (int win = 0; win < dkgk::SEAT_ENC_WINDOWS; win++)  // the kernel's loop (k_seat_enc_mul)
    digits[win] = (int8_t)dkgk::seat_enc_digit(dkgk::seat_enc_bits(w[win >> 4], win), win, carry);
  *windows = dkgk::SEAT_ENC_WINDOWS;
  return DKG_OK;
}
int dkg_split_digits(size_t n, size_t L, int pieces, int mode, int8_t* digits, int16_t* top) {
  if (!n || !L || pieces < 2 || pieces > (int)SHORT_MAX || mode < 0 || mode > 3 || mode == 1 || !digits || !top)
    return DKG_E_ARG;
  try {
    const size_t K = (size_t)pieces;
    const bool jsf = mode != 3 && jsf_built(K);
    std::vector<uint8_t> m;
    std::vector<int8_t> sg;
    short_vectors(n, L, K, m, sg, jsf);
    std::vector<uint32_t> hd;
    std::vector<int16_t> ht;
    if (!short_digit_words(n, K, jsf, m, sg, hd, ht, nullptr)) return DKG_E_ARG;
    for (size_t j = 0; j < n; j++) {
      top[j] = ht[j];
      for (size_t u = 0; u < K; u++)
        for (size_t b = 0; b < 256; b++)
          digits[(j * K + u) * 256 + b] = (int8_t)(hd[(u / 4) * 256 * n + 256 * j + b] >> (8 * (u % 4)));
    }
  } catch (const std::exception&) {
    return DKG_E_NOMEM;
  }
  return DKG_OK;
}

double dkg_split_model_ms(size_t columns, size_t n, size_t t, int pieces) {
  if (pieces < 1 || t + 1 < (size_t)pieces) return -1;
  return split_model_ms(columns, n, t + 1, (size_t)pieces);
}

int dkg_stepping_lane_map(int lanes, int seg_len, int nseg, int last_len, int lane, int out[3]) {
  if (lanes <= 0 || lanes % 64 || lanes > 512 || lane < 0 || lane >= lanes || !out) return -1;
  const int B = step_band(lanes, seg_len, nseg, last_len);
  if (!B) return 0;
  const StepLane m = step_band_lane(lane, B, lanes);
  out[0] = m.seg, out[1] = m.q, out[2] = m.next;
  return B;
}

size_t dkg_split_len(size_t columns, size_t n, size_t t, int pieces) {
  if (pieces < 1 || t + 1 < (size_t)pieces) return 0;
  return split_len(columns, n, t + 1, (size_t)pieces);
}

int dkg_ctx_set_overlap(dkg_ctx* ctx, int on) {
  if (!ctx) return DKG_E_ARG;
  ctx->overlap = on != 0;
  return DKG_OK;
}

int dkg_env_check(size_t threshold, size_t nr_members) {
  // committee.rs:73: assert!(threshold < (nr_members + 1) / 2)
  if (nr_members == 0 || !(threshold < (nr_members + 1) / 2)) return DKG_E_ARG;
  return DKG_OK;
}

int dkg_env_init(dkg_ctx* ctx, size_t threshold, size_t nr_members, const uint8_t* ck, size_t ck_len,
                 uint8_t h_out[32]) {
  int rc = dkg_env_check(threshold, nr_members);
  if (rc != DKG_OK) {
    if (ctx) ctx->err = "threshold must be < (nr_members + 1) / 2 (committee.rs:73)";
    return rc;
  }
  return guarded(ctx, [&] {
    // CommitmentKey::generate: h = RistrettoPoint::hash_from_bytes::<Blake2b>(ck) (commitment.rs:13-17)
    uint8_t hash[64];
    dkgh::blake2b(hash, 64, ck, ck_len);
    uint32_t* in = buf<uint32_t>(ctx, "h_in", 64);
    uint32_t* ext = buf<uint32_t>(ctx, "h_ext", PTB);
    uint32_t* comp = buf<uint32_t>(ctx, "h_comp", 32);
    h2d(ctx, in, hash, 64);
    dkgk::from_uniform(in, ext, ctx->stream);
    dkgk::encode_points(ext, 1, 1, comp, ctx->stream);
    check_launch(ctx);
    d2h(ctx, ctx->h, comp, 32);
    sync(ctx);
    bool ok = false;
    comb_for_point(ctx, ctx->h, ctx->tab_h, &ok, ctx->tab_hw);
    if (!ok) return DKG_E_DEVICE;
    ctx->have_h = true;
    ctx->threshold = threshold;
    ctx->nr_members = nr_members;
    if (h_out) memcpy(h_out, ctx->h, 32);
    return DKG_OK;
  });
}

int dkg_msm_batch(dkg_ctx* ctx, size_t B, size_t N, const uint8_t* scalars, const uint8_t* points, uint8_t* out) {
  return guarded(ctx, [&] {
    if (B == 0) return DKG_OK;
    uint32_t* sc = upload_scalars(ctx, "msm_sc", scalars, B * N);
    uint32_t* pc = buf<uint32_t>(ctx, "msm_pc", 32 * B * N);
    uint32_t* pe = buf<uint32_t>(ctx, "msm_pe", PTB * B * N);
    uint8_t* ok = buf<uint8_t>(ctx, "msm_ok", B * N);
    h2d(ctx, pc, points, 32 * B * N);
    dkgk::decode_points(pc, B * N, pe, B * N, ok, ctx->stream);
    uint32_t* oe = buf<uint32_t>(ctx, "msm_oe", PTB * B);
    uint32_t* oc = buf<uint32_t>(ctx, "msm_oc", 32 * B);
    uint32_t* mt = buf<uint32_t>(ctx, "msm_tab", 4 * 15 * PT_WORDS_H * B * N);
  dkgk::msm_batch(B, N, sc, pe, B * N, mt, oe, ctx->stream);
    dkgk::encode_points(oe, B, B, oc, ctx->stream);
    check_launch(ctx);
    std::vector<uint8_t> okh(B * N);
    d2h(ctx, okh.data(), ok, B * N);
    d2h(ctx, out, oc, 32 * B);
    sync(ctx);
    for (auto v : okh)
      if (!v) {
        ctx->err = "msm: a point failed to decode";
        return DKG_E_DECODE;
      }
    return DKG_OK;
  });
}

int dkg_fixed_base_batch(dkg_ctx* ctx, const uint8_t base[32], size_t count, const uint8_t* scalars, uint8_t* out) {
  return guarded(ctx, [&] {
    if (count == 0) return DKG_OK;
    const uint32_t* tab = ctx->tab_gw;
    // the generator and the commitment key have their combs already; another base's comb (470 MB,
    // ~1M entry threads) is built once and kept while the caller passes the same base bytes
    if (base && memcmp(base, BASEPOINT, 32) == 0) {
      base = nullptr;
    } else if (base && ctx->have_h && ctx->tab_hw && memcmp(base, ctx->h, 32) == 0) {
      tab = ctx->tab_hw;
      base = nullptr;
    }
    if (base) {
      uint32_t* t = buf<uint32_t>(ctx, "fb_tabw", COMBW_BYTES);
      if (!ctx->fb_valid || memcmp(ctx->fb_base, base, 32) != 0) {
        ctx->fb_valid = false;
        bool ok = false;
        comb_for_point(ctx, base, nullptr, &ok, t);
        if (!ok) {
          ctx->err = "fixed_base: base point failed to decode";
          return DKG_E_DECODE;
        }
        memcpy(ctx->fb_base, base, 32);
        ctx->fb_valid = true;
      }
      tab = t;
    }
    uint32_t* sc = upload_scalars(ctx, "fb_sc", scalars, count);
    uint32_t* oe = buf<uint32_t>(ctx, "fb_oe", PTB * count);
    uint32_t* oc = buf<uint32_t>(ctx, "fb_oc", 32 * count);
    dkgk::fixed_base(count, sc, tab, oe, ctx->stream);
    dkgk::encode_points(oe, count, count, oc, ctx->stream);
    check_launch(ctx);
    d2h(ctx, out, oc, 32 * count);
    sync(ctx);
    return DKG_OK;
  });
}

int dkg_poly_eval_batch(dkg_ctx* ctx, size_t D, size_t N, const uint8_t* coeffs, size_t M, const uint32_t* xs,
                        uint8_t* out) {
  return guarded(ctx, [&] {
    if (D == 0 || M == 0) return DKG_OK;
    if (N == 0) return DKG_E_ARG;
    for (size_t m = 0; m < M; m++)
      if (xs[m] >= (1u << 24)) {
        ctx->err = "poly_eval: evaluation points must be < 2^24";
        return DKG_E_ARG;
      }
    uint32_t* c = upload_scalars(ctx, "pe_c", coeffs, D * N);
    uint32_t* x = buf<uint32_t>(ctx, "pe_x", 4 * M);
    uint32_t* o = buf<uint32_t>(ctx, "pe_o", 32 * D * M);
    h2d(ctx, x, xs, 4 * M);
    dkgk::poly_eval(D, N, c, M, x, o, ctx->stream);
    check_launch(ctx);
    d2h(ctx, out, o, 32 * D * M);
    sync(ctx);
    return DKG_OK;
  });
}

int dkg_zero_tests(dkg_ctx* ctx, size_t count, const uint32_t* limbs, uint8_t* out) {
  return guarded(ctx, [&] {
    if (count == 0) return DKG_OK;
    if (!limbs || !out) return DKG_E_ARG;
    uint32_t* dl = buf<uint32_t>(ctx, "zt_limbs", 40 * count);
    uint8_t* od = buf<uint8_t>(ctx, "zt_out", 3 * count);
    h2d(ctx, dl, limbs, 40 * count);
    dkgk::zero_tests(count, dl, od, ctx->stream);
    check_launch(ctx);
    d2h(ctx, out, od, 3 * count);
    sync(ctx);
    return DKG_OK;
  });
}

int dkg_fe_ops(dkg_ctx* ctx, int flavour, int op, size_t count, const uint32_t* in, uint32_t* out) {
  return guarded(ctx, [&] {
    size_t win, wout;
    if ((flavour != 1 && flavour != 2) || !dkgk::fe_ops_shape(op, &win, &wout)) return DKG_E_ARG;
    if (count == 0) return DKG_OK;
    if (!in || !out) return DKG_E_ARG;
    uint32_t* di = buf<uint32_t>(ctx, "fo_in", 4 * win * count);
    uint32_t* od = buf<uint32_t>(ctx, "fo_out", 4 * wout * count);
    h2d(ctx, di, in, 4 * win * count);
    (flavour == 2 ? dkgk_ilp::fe_ops : dkgk::fe_ops)(op, count, di, od, ctx->stream);
    check_launch(ctx);
    d2h(ctx, out, od, 4 * wout * count);
    sync(ctx);
    return DKG_OK;
  });
}

int dkg_sc_ops(dkg_ctx* ctx, int op, size_t count, const uint32_t* in, uint32_t* out) {
  return guarded(ctx, [&] {
    size_t win, wout;
    if (!dkgk::sc_ops_shape(op, &win, &wout)) return DKG_E_ARG;
    if (count == 0) return DKG_OK;
    if (!in || !out) return DKG_E_ARG;
    if (op == dkgk::SC_OP_LAZY)
      for (size_t e = 0; e < count; e++)
        if (in[e * win + 10] > dkgk::sc_ops_lazy_steps()) {
          ctx->err = "sc_ops: more lazy steps than SC_LAZY_STEPS";
          return DKG_E_ARG;
        }
    uint32_t* di = buf<uint32_t>(ctx, "so_in", 4 * win * count);
    uint32_t* od = buf<uint32_t>(ctx, "so_out", 4 * wout * count);
    h2d(ctx, di, in, 4 * win * count);
    dkgk::sc_ops(op, count, di, od, ctx->stream);
    check_launch(ctx);
    d2h(ctx, out, od, 4 * wout * count);
    sync(ctx);
    return DKG_OK;
  });
}

int dkg_points_valid_batch(dkg_ctx* ctx, size_t count, const uint8_t* points, uint8_t* ok) {
  return guarded(ctx, [&] {
    if (count == 0) return DKG_OK;
    uint32_t* pc = buf<uint32_t>(ctx, "pv_c", 32 * count);
    uint32_t* pe = buf<uint32_t>(ctx, "pv_e", PTB * count);
    uint8_t* od = buf<uint8_t>(ctx, "pv_ok", count);
    h2d(ctx, pc, points, 32 * count);
    dkgk::decode_points(pc, count, pe, count, od, ctx->stream);
    check_launch(ctx);
    d2h(ctx, ok, od, count);
    sync(ctx);
    return DKG_OK;
  });
}

int dkg_share_gen(dkg_ctx* ctx, size_t D, size_t n, size_t t, const uint8_t* a, const uint8_t* b, uint8_t* E,
                  uint8_t* A, uint8_t* s, uint8_t* s_prime) {
  return guarded(ctx, [&] {
    int rc = need_env(ctx);
    if (rc) return rc;
    if (D == 0) return DKG_OK;
    const size_t N = t + 1;
    uint32_t* da = upload_scalars(ctx, "sg_a", a, D * N);
    uint32_t* db = upload_scalars(ctx, "sg_b", b, D * N);
    uint32_t* Ec = buf<uint32_t>(ctx, "sg_E", 32 * D * N);
    uint32_t* Ac = buf<uint32_t>(ctx, "sg_A", 32 * D * N);
    uint32_t* ds = buf<uint32_t>(ctx, "sg_s", 32 * D * n);
    uint32_t* dsp = buf<uint32_t>(ctx, "sg_sp", 32 * D * n);
    round1_device(ctx, D, n, t, da, db, Ec, Ac, ds, dsp);
    if (E) d2h(ctx, E, Ec, 32 * D * N);
    if (A) d2h(ctx, A, Ac, 32 * D * N);
    if (s) d2h(ctx, s, ds, 32 * D * n);
    if (s_prime) d2h(ctx, s_prime, dsp, 32 * D * n);
    sync(ctx);
    return DKG_OK;
  });
}

int dkg_share_gen_device(dkg_ctx* ctx, size_t D, size_t n, size_t t, const void* d_a, const void* d_b, void* d_E,
                         void* d_A, void* d_s, void* d_s_prime) {
  return guarded(ctx, [&] {
    int rc = need_env(ctx);
    if (rc) return rc;
    if (!d_a || !d_b || !d_s || !d_s_prime) return DKG_E_ARG;
    if (D == 0) return DKG_OK;
    const size_t N = t + 1;
    uint32_t* Ec = d_E ? (uint32_t*)d_E : buf<uint32_t>(ctx, "sgd_E", 32 * D * N);
    uint32_t* Ac = d_A ? (uint32_t*)d_A : buf<uint32_t>(ctx, "sgd_A", 32 * D * N);
    round1_device(ctx, D, n, t, (const uint32_t*)d_a, (const uint32_t*)d_b, Ec, Ac, (uint32_t*)d_s,
                  (uint32_t*)d_s_prime, d_E || d_A);
    sync(ctx);
    return DKG_OK;
  });
}

int dkg_verify_pairs(dkg_ctx* ctx, size_t n, size_t t, int round, size_t d0, size_t d1, const uint8_t* C,
                     const uint8_t* s, const uint8_t* s_prime, uint8_t* decision) {
  return guarded(ctx, [&] {
    if ((round != 2 && round != 4) || d1 < d0 || d1 > n) return DKG_E_ARG;
    if (round == 2) {
      int rc = need_env(ctx);
      if (rc) return rc;
      if (!s_prime) return DKG_E_ARG;
    }
    const size_t D = d1 - d0, N = t + 1;
    if (D == 0) return DKG_OK;
    uint32_t* Cc = buf<uint32_t>(ctx, "vp_C", 32 * D * N);
    h2d(ctx, Cc, C, 32 * D * N);
    uint32_t* ds = upload_scalars(ctx, "vp_s", s, D * n);
    uint32_t* dsp = round == 2 ? upload_scalars(ctx, "vp_sp", s_prime, D * n) : nullptr;
    uint8_t* dec = buf<uint8_t>(ctx, "vp_dec", D * n);
    verify_one(ctx, n, t, round, D, d0, Cc, ds, dsp, dec, false);
    d2h(ctx, decision, dec, D * n);
    sync(ctx);
    return DKG_OK;
  });
}

int dkg_verify_receiver(dkg_ctx* ctx, size_t n, size_t t, int round, size_t j, const uint8_t* C, const uint8_t* s,
                        const uint8_t* s_prime, uint8_t* decision) {
  return guarded(ctx, [&] {
    if ((round != 2 && round != 4) || j >= n) return DKG_E_ARG;
    ctx->last_step_flags = nullptr;  // Horner per receiver: no stepping tables
    ctx->last_step_flag_words = 0;
    ctx->last_bflags = nullptr;
    ctx->last_bflag_words = 0;
    if (round == 2) {
      int rc = need_env(ctx);
      if (rc) return rc;
      if (!s_prime) return DKG_E_ARG;
    }
    const size_t N = t + 1, npad = pad64(n);
    uint32_t* Cc = buf<uint32_t>(ctx, "vr_C", 32 * n * N);
    h2d(ctx, Cc, C, 32 * n * N);
    uint32_t* Cext = buf<uint32_t>(ctx, "Cext", PTB * n * N);
    uint8_t* pok = buf<uint8_t>(ctx, "pok", n * N);
    uint8_t* dok = buf<uint8_t>(ctx, "dok", n);
    uint32_t* Cpm = buf<uint32_t>(ctx, "Cpm", PTB * N * npad);
    dkgk::decode_points(Cc, n * N, Cext, n * N, pok, ctx->stream);
    dkgk::dealer_ok(n, N, pok, dok, ctx->stream);
    dkgk::to_position_major(n, N, npad, Cext, Cpm, ctx->stream);
    uint32_t* R = buf<uint32_t>(ctx, "vr_R", PTB * n);
    dkgk::horner(n, npad, N, Cpm, (uint32_t)(j + 1), 1, R, ctx->stream);  // committee.rs:287-296, one party
    uint32_t* ds = upload_scalars(ctx, "vr_s", s, n);
    uint32_t* dsp = round == 2 ? upload_scalars(ctx, "vr_sp", s_prime, n) : nullptr;
    uint8_t* dec = buf<uint8_t>(ctx, "vr_dec", n);
    dkgk::check(n, 1, 0, j, n, round, ds, dsp, R, ctx->tab_gw, ctx->tab_hw, dok, dec, ctx->stream);
    check_launch(ctx);
    d2h(ctx, decision, dec, n);
    sync(ctx);
    return DKG_OK;
  });
}

int dkg_ceremony_run_device(dkg_ctx* ctx, size_t n, size_t t, const void* d_a, const void* d_b,
                            dkg_ceremony_out* out) {
  return guarded(ctx, [&] {
    const int rc = ceremony_args(ctx, n, t, {out});
    if (rc) return rc;
    const size_t N = t + 1;
    HCK(hipEventRecord(ctx->ev[0], ctx->stream));
    const Commitments cm = commitment_rows(ctx, n, N);
    uint32_t* ds = buf<uint32_t>(ctx, "cer_s", 32 * n * n);
    uint32_t* dsp = buf<uint32_t>(ctx, "cer_sp", 32 * n * n);
#ifdef DKG_NO_R1_OVERLAP
    round1_device(ctx, n, n, t, (const uint32_t*)d_a, (const uint32_t*)d_b, cm.E, cm.A, ds, dsp, false);
#else
    // with one stream (the bench's serialised roofline pass) the phases stay back to back
    round1_device(ctx, n, n, t, (const uint32_t*)d_a, (const uint32_t*)d_b, cm.E, cm.A, ds, dsp, false, ctx->nsub > 1);
#endif
    HCK(hipEventRecord(ctx->ev[1], ctx->stream));
    ExtScope ext(ctx, n, N);
    receivers_rounds(ctx, n, t, cm.E, cm.A, ds, dsp, out, false);  // small outputs only
    ceremony_times(ctx, out, true);
    return DKG_OK;
  });
}

int dkg_ceremony_run(dkg_ctx* ctx, size_t n, size_t t, const uint8_t* a, const uint8_t* b, dkg_ceremony_out* out) {
  return guarded(ctx, [&] {
    const int rc = ceremony_args(ctx, n, t, {out});
    if (rc) return rc;
    const size_t N = t + 1;
    uint32_t* da = upload_scalars(ctx, "cer_a", a, n * N);
    uint32_t* db = upload_scalars(ctx, "cer_b", b, n * N);
    HCK(hipEventRecord(ctx->ev[0], ctx->stream));
    const Commitments cm = commitment_rows(ctx, n, N);
    uint32_t* ds = buf<uint32_t>(ctx, "cer_s", 32 * n * n);
    uint32_t* dsp = buf<uint32_t>(ctx, "cer_sp", 32 * n * n);
    round1_device(ctx, n, n, t, da, db, cm.E, cm.A, ds, dsp);
    HCK(hipEventRecord(ctx->ev[1], ctx->stream));
    if (out->E) d2h(ctx, out->E, cm.E, 32 * n * N);
    if (out->A) d2h(ctx, out->A, cm.A, 32 * n * N);
    if (out->s) d2h(ctx, out->s, ds, 32 * n * n);
    if (out->s_prime) d2h(ctx, out->s_prime, dsp, 32 * n * n);
    ExtScope ext(ctx, n, N);
    receivers_rounds(ctx, n, t, cm.E, cm.A, ds, dsp, out, true);
    ceremony_times(ctx, out, true);
    return DKG_OK;
  });
}

int dkg_ceremony_verify(dkg_ctx* ctx, size_t n, size_t t, const uint8_t* E, const uint8_t* A, const uint8_t* s,
                        const uint8_t* s_prime, dkg_ceremony_out* out) {
  return guarded(ctx, [&] {
    const int rc = ceremony_args(ctx, n, t, {out, E, A, s, s_prime});
    if (rc) return rc;
    CeremonyInput in;
    in.E = E, in.A = A, in.s = s, in.s_prime = s_prime;
    return verify_ceremony(ctx, n, t, in, out);
  });
}

int dkg_ceremony_verify_fetched(dkg_ctx* ctx, size_t n, size_t t, const uint8_t* E, const uint8_t* A,
                                const uint8_t* s, const uint8_t* s_prime, const uint8_t* fetched1,
                                const uint8_t* fetched3, dkg_ceremony_out* out) {
  return guarded(ctx, [&] {
    const int rc = ceremony_args(ctx, n, t, {out, E, A, s, s_prime, fetched1, fetched3});
    if (rc) return rc;
    CeremonyInput in;
    in.E = E, in.A = A, in.s = s, in.s_prime = s_prime, in.fetched1 = fetched1, in.fetched3 = fetched3;
    return verify_ceremony(ctx, n, t, in, out);
  });
}

}  // extern "C"

// ---- the proven-complaint rule on a dealer shard (dkg_ceremony_shard_verify_proven_device, _full_proven_device)
// Every fact that decides a complaint against dealer i lives on the rank that owns i: its E and A rows,
// its e1 / ct items and their decode mask, its round-2 qualification, its fetched3 bit; the accusers'
// keys are the pk [n] every rank takes.  So each rank verifies the complaints against its own dealers
// (d0 < accused <= d0 + D, in their relative input order) and no exchange precedes round 3.
// The owned complaints go up once, before the rounds: one pinned staging block
//   accuser4 | row4 | accuser2 | row2 | share4 [C4][8] | randomness4 [C4][8] | proofs [C2][48]
// with row = accused - d0, the accused's 1-based row among the rank's dealers.
struct ShardProven {
  bool full = false;  // encrypted shares: round 2 by the proven complaints too (else the rejection rule)
  // the ceremony's broadcast complaint lists (host, as every rank receives them) and the intake masks [D]
  const uint8_t* pk = nullptr;
  size_t C2 = 0, C4 = 0;
  const uint32_t *accuser2 = nullptr, *accused2 = nullptr, *accuser4 = nullptr, *accused4 = nullptr;
  const uint8_t *proofs = nullptr, *share4 = nullptr, *randomness4 = nullptr;
  const uint8_t *fetched1 = nullptr, *fetched3 = nullptr;
  int32_t *verdict2 = nullptr, *verdict4 = nullptr;
  size_t flag_rows = 0;
  void *d_flags = nullptr, *d_dissent = nullptr;
  // the owned complaints: their places in the input lists, and the host copies the fallback's
  // complaint_evals reads (acc / row per complaint; for round 4 per evaluation item, E then A)
  std::vector<uint32_t> own2, own4, acc2h, row2h, acc4h, row4h, idx4h, item4h;
  const uint32_t *dacc2 = nullptr, *drow2 = nullptr, *dacc4 = nullptr, *drow4 = nullptr;
  const uint32_t *dsh = nullptr, *drn = nullptr, *dprf = nullptr, *dpk = nullptr;
  const uint8_t *df1 = nullptr, *df3 = nullptr;
  int32_t *hver2 = nullptr, *hver4 = nullptr;  // pinned copies of the owned complaints' verdicts
  ComplaintEvals ev2, ev4;                     // the fallback's staging, alive until the call's sync
};

void shard_proven_upload(dkg_ctx* ctx, size_t n, size_t d0, size_t D, ShardProven& sp) {
  auto own = [&](size_t C, const uint32_t* accuser, const uint32_t* accused, std::vector<uint32_t>& pos,
                 std::vector<uint32_t>& acc, std::vector<uint32_t>& row) {
    for (size_t c = 0; c < C; c++)
      if (accused[c] > d0 && accused[c] <= d0 + D) {
        pos.push_back((uint32_t)c);
        acc.push_back(accuser[c]);
        row.push_back(accused[c] - (uint32_t)d0);
      }
  };
  own(sp.C4, sp.accuser4, sp.accused4, sp.own4, sp.acc4h, sp.row4h);
  if (sp.full) own(sp.C2, sp.accuser2, sp.accused2, sp.own2, sp.acc2h, sp.row2h);
  const size_t o2 = sp.own2.size(), o4 = sp.own4.size();
  for (size_t k = 0; k < o4; k++) {  // items 2k, 2k + 1: rows i and D + i of the [2D] decoded rows
    sp.idx4h.insert(sp.idx4h.end(), {sp.acc4h[k], sp.acc4h[k]});
    sp.item4h.insert(sp.item4h.end(), {sp.row4h[k], (uint32_t)D + sp.row4h[k]});
  }
  const size_t words = 2 * o4 + 2 * o2 + 16 * o4 + 48 * o2;
  uint32_t* h = hbuf<uint32_t>(ctx, "hb.sp_in", 4 * words);
  uint32_t* d = buf<uint32_t>(ctx, "sp.in", 4 * words);
  size_t at = 0;
  auto put = [&](const void* src, size_t cnt) {
    const uint32_t* p = d + at;
    if (cnt) memcpy(h + at, src, 4 * cnt);
    at += cnt;
    return p;
  };
  sp.dacc4 = put(sp.acc4h.data(), o4);
  sp.drow4 = put(sp.row4h.data(), o4);
  sp.dacc2 = put(sp.acc2h.data(), o2);
  sp.drow2 = put(sp.row2h.data(), o2);
  sp.dsh = d + at;
  for (size_t k = 0; k < o4; k++) put(sp.share4 + 32 * (size_t)sp.own4[k], 8);
  sp.drn = d + at;
  for (size_t k = 0; k < o4; k++) put(sp.randomness4 + 32 * (size_t)sp.own4[k], 8);
  sp.dprf = d + at;
  for (size_t k = 0; k < o2; k++) put(sp.proofs + 192 * (size_t)sp.own2[k], 48);
  h2d(ctx, d, h, 4 * words);
  if (sp.full) {
    uint32_t* dpk = buf<uint32_t>(ctx, "sp.pk", 32 * n);
    h2d(ctx, dpk, sp.pk, 32 * n);
    sp.dpk = dpk;
  }
  sp.df1 = upload_mask(ctx, "sp.f1", sp.fetched1, D);
  sp.df3 = upload_mask(ctx, "sp.f3", sp.fetched3, D);
  sp.hver2 = hbuf<int32_t>(ctx, "hb.sp_ver2", 4 * o2);
  sp.hver4 = hbuf<int32_t>(ctx, "hb.sp_ver4", 4 * o4);
}

// A rank without dealers (world_size > n / 2 leaves some): no flags, no dissent
void shard_complaints_none(dkg_ctx* ctx, size_t n, ShardProven& sp) {
  if (sp.flag_rows) HCK(hipMemsetAsync(sp.d_flags, 0, 4 * sp.flag_rows, ctx->stream));
  if (sp.d_dissent) HCK(hipMemsetAsync(sp.d_dissent, 0, 4 * n, ctx->stream));
  ctx->last_complaint_eval = 0;
}

// The complaint stage of a rank, queued on ctx->stream after its rounds' checks; no host synchronisation.
// Ec, Ac [D][N][8] the rank's commitments, e1c / ctc its ciphertexts (full mode), dec2 [D][n] the round-2
// rows just decided.  Out: qm [D] the rank's dealers' qualified mask (rej its complement) -- full mode: the
// row is not MISSING and no complaint against it has verdict 0; else the rejection rule -- the flag words,
// the dissent partial, and the verdicts in sp.hver2 / hver4.
// Evaluation source 3, "the calling pass": when the rounds ran fused in group-check mode their R holds
// P^E_i(j) and P^A_i(j) of every receiver of every dealer of the rank at once, and the complaints'
// items are elements of it (k_shard_ridx) -- no Horner walk, no second set of tables; the rows' validity
// is the pass's own decode flags.  Otherwise (protocol-order rounds, interpolation, a forced
// dkg_ctx_set_complaint_eval, or an R too large for 31-bit elements): the rows are decoded once more and
// complaint_evals decides per accused row as in dkg_complaints_verify.
void shard_complaints(dkg_ctx* ctx, size_t n, size_t t, size_t D, const uint32_t* Ec, const uint32_t* Ac,
                      const uint32_t* e1c, const uint32_t* ctc, const uint8_t* dec2, uint8_t* rej, uint8_t* qm,
                      ShardProven& sp) {
  const size_t N = t + 1, C2 = sp.own2.size(), C4 = sp.own4.size();
  hipStream_t st = ctx->stream;
  const size_t npad = (D + 63) / 64 * 128;
  const bool pass = ctx->overlap && ctx->verify_mode == 0 && ctx->last_R && ctx->last_dok_nseg == 2 &&
                    ctx->last_npad == npad && (uint64_t)npad * n < (1ull << 31);
  const bool src3 = pass && ctx->complaint_eval == 0;
  const uint32_t *passR = ctx->last_R, *pass_scale = ctx->last_scale;
  uint8_t* rowok = buf<uint8_t>(ctx, "sp.rowok", 2 * D);  // the E rows, then the A rows, decode
  const uint32_t *EA = nullptr, *EAext = nullptr, *Rh0 = nullptr;
  if (src3) {
    uint8_t* raw = buf<uint8_t>(ctx, "sp.rawdok", npad);  // the columns' decode flags without the dealer masks
    dkgk::dealer_ok(npad, N, ctx->last_pok, raw, st);
    dkgk::segment_mask(D, 2, 0, raw, rowok, st);
    dkgk::segment_mask(D, 2, 1, raw, rowok + D, st);
    uint32_t* id = buf<uint32_t>(ctx, "sp.Rh0", PTB);  // what a complaint against an undecodable row reads
    dkgk::fill_identity(1, id, st);
    Rh0 = id;
  } else {
    uint32_t* ea = buf<uint32_t>(ctx, "sp.EA", 32 * 2 * D * N);
    uint32_t* ext = buf<uint32_t>(ctx, "sp.EAext", PTB * 2 * D * N);
    uint8_t* pok = buf<uint8_t>(ctx, "sp.pok", 2 * D * N);
    HCK(hipMemcpyAsync(ea, Ec, 32 * D * N, hipMemcpyDeviceToDevice, st));
    HCK(hipMemcpyAsync(ea + 8 * D * N, Ac, 32 * D * N, hipMemcpyDeviceToDevice, st));
    dkgk::decode_points(ea, 2 * D * N, ext, 2 * D * N, pok, st);
    dkgk::dealer_ok(2 * D, N, pok, rowok, st);
    EA = ea, EAext = ext;
  }
  sp.ev2 = ComplaintEvals{};
  sp.ev4 = ComplaintEvals{};
  uint8_t* proven4 = buf<uint8_t>(ctx, "sp.proven4", D);
  HCK(hipMemsetAsync(proven4, 0, D, st));
  int32_t* dver2 = buf<int32_t>(ctx, "sp.verdict2", 4 * C2);
  int32_t* dver4 = buf<int32_t>(ctx, "sp.verdict4", 4 * C4);
  uint8_t *cmask = nullptr, *pair = nullptr;
  // ---- round 2 (k_cv_*): the pair dealer i sent accuser j out of the rank's own ciphertexts
  if (sp.full) {
    cmask = buf<uint8_t>(ctx, "sp.cmask", D);
    pair = buf<uint8_t>(ctx, "sp.pair", D * n);
    HCK(hipMemsetAsync(cmask, 1, D, st));
    HCK(hipMemsetAsync(pair, 0, D * n, st));
    if (C2) {
      uint32_t* denc = buf<uint32_t>(ctx, "sp.enc", 128 * C2);
      dkgk::gather_enc(C2, n, sp.drow2, sp.dacc2, e1c, ctc, denc, st);
      const Announcements an = complaint_announcements(ctx, C2, sp.dacc2, sp.dpk, denc, sp.dprf, st);
      const uint32_t *ridx, *Rh, *Rt, *scale;
      if (src3) {
        uint32_t* r = buf<uint32_t>(ctx, "sp.ridx2", 4 * C2);
        dkgk::shard_ridx(C2, 1, D, n, sp.drow2, sp.dacc2, rowok, r, st);
        ridx = r, Rh = Rh0, Rt = passR, scale = pass_scale;
      } else {
        complaint_evals(ctx, n, t, 2 * D, C2, sp.acc2h.data(), sp.row2h.data(), sp.dacc2, sp.drow2, EA, EAext, sp.ev2);
        ridx = sp.ev2.dridx, Rh = sp.ev2.Rh, Rt = sp.ev2.Rt, scale = sp.ev2.scale;
      }
      uint8_t* eq = buf<uint8_t>(ctx, "sp.eq2", 2 * C2);
      dkgk::cv_check(C2, sp.dacc2, an.p12, ridx, Rh, Rt, scale, ctx->tab_gw, ctx->tab_hw, eq, st);
      dkgk::cv_final(C2, sp.dacc2, sp.drow2, sp.dpk, denc, sp.dprf, an.a1c, an.a2c, an.ppok, rowok, sp.df1, eq, dver2, st);
      dkgk::proven_masks(C2, n, sp.drow2, sp.dacc2, dver2, 0, nullptr, nullptr, cmask, pair, proven4, st);
    }
    dkgk::qualified_complaints(D, n, dec2, cmask, rej, qm, st);
  } else {
    dkgk::row_reject(D, n, dec2, rej, st);
    dkgk::mask_not_and(D, rej, nullptr, qm, st);
  }
  // ---- round 4 (k_c3_*): the rank's qualified mask gives IGNORED on the device (committee.rs:639)
  if (C4) {
    uint32_t* sr = buf<uint32_t>(ctx, "sp.sr", 32 * 2 * C4);
    uint32_t* acc2x = buf<uint32_t>(ctx, "sp.acc2x", 4 * 2 * C4);
    uint32_t* acd2x = buf<uint32_t>(ctx, "sp.acd2x", 4 * 2 * C4);
    dkgk::c3_prep(C4, D, sp.dacc4, sp.drow4, sp.dsh, sp.drn, sr, acc2x, acd2x, st);
    const uint32_t *ridx, *Rh, *Rt, *scale;
    if (src3) {
      uint32_t* r = buf<uint32_t>(ctx, "sp.ridx4", 4 * 2 * C4);
      dkgk::shard_ridx(C4, 2, D, n, sp.drow4, sp.dacc4, rowok, r, st);
      ridx = r, Rh = Rh0, Rt = passR, scale = pass_scale;
    } else {
      complaint_evals(ctx, n, t, 2 * D, 2 * C4, sp.idx4h.data(), sp.item4h.data(), acc2x, acd2x, EA, EAext, sp.ev4);
      ridx = sp.ev4.dridx, Rh = sp.ev4.Rh, Rt = sp.ev4.Rt, scale = sp.ev4.scale;
    }
    uint8_t* eq = buf<uint8_t>(ctx, "sp.eq4", 2 * C4);
    dkgk::c3_check(C4, sp.dacc4, sr, ridx, Rh, Rt, scale, ctx->tab_gw, ctx->tab_hw, eq, st);
    dkgk::c3_final(C4, D, sp.drow4, sp.drow4, rowok, qm, sp.df3, eq, dver4, st);
    dkgk::proven_masks(0, n, nullptr, nullptr, nullptr, C4, sp.drow4, dver4, cmask, pair, proven4, st);
  }
  dkgk::shard_flags(D, sp.flag_rows, cmask, proven4, rowok + D, sp.df3, (uint32_t*)sp.d_flags, st);
  if (sp.d_dissent) dkgk::shard_dissent(D, n, dec2, pair, (int32_t*)sp.d_dissent, st);
  d2h(ctx, sp.hver2, dver2, 4 * C2);
  d2h(ctx, sp.hver4, dver4, 4 * C4);
  if (src3) {
    ctx->last_complaint_eval = 3;
  } else {
    const bool horner = !sp.ev2.hl.empty() || !sp.ev4.hl.empty(), tables = !sp.ev2.rows.empty() || !sp.ev4.rows.empty();
    ctx->last_complaint_eval = ctx->complaint_eval == 4 ? 4
                               : horner && tables       ? 12
                               : tables                 ? 2
                               : horner                 ? 1
                               : ctx->complaint_eval == 2 ? 2
                                                          : 1;
  }
}

// After the call's sync: every complaint the rank does not own reads DKG_COMPLAINT_NOT_OWNED, the owned
// ones their verdicts
void shard_proven_verdicts(const ShardProven& sp) {
  for (size_t c = 0; c < sp.C2; c++) sp.verdict2[c] = DKG_COMPLAINT_NOT_OWNED;
  for (size_t c = 0; c < sp.C4; c++) sp.verdict4[c] = DKG_COMPLAINT_NOT_OWNED;
  for (size_t k = 0; k < sp.own2.size(); k++) sp.verdict2[sp.own2[k]] = sp.hver2[k];
  for (size_t k = 0; k < sp.own4.size(); k++) sp.verdict4[sp.own4[k]] = sp.hver4[k];
}

// One rank's call of a dealer-sharded ceremony on its dealers [d0, d1), as the pointers of the C ABI
// (null = absent; device pointers unless marked host), in the manner of CeremonyInput.  Generate mode is
// a != nullptr, full mode is sk != nullptr, and the proven rule follows the presence of `proven`, not
// C > 0.  Layouts as dkg_ceremony_shard_device documents them.
struct ShardInput {
  const void *a = nullptr, *b = nullptr;        // the dealers' coefficients (generate), or
  const void *E = nullptr, *A = nullptr;        //   the received commitments
  const void *s = nullptr, *s_prime = nullptr;  // the received plaintext shares, or
  const void *e1 = nullptr, *ct = nullptr;      //   the received ciphertexts, or
  const void* r = nullptr;                      //   the encryption randomness (generate, full mode)
  void *e1_out = nullptr, *ct_out = nullptr;    //     and where its ciphertexts go (optional)
  const uint8_t *sk = nullptr, *pk = nullptr;   // host: the members' keys (full mode)
  ShardProven* proven = nullptr;                // the complaint lists, the intake masks, flags and verdicts
  void *dec2 = nullptr, *dec4 = nullptr, *A0 = nullptr, *partial = nullptr;
  double* ms_total = nullptr;
};

// What the share stage of shard_ceremony hands the rounds: E/A compressed [D][N][32], s/sp canonical
// [D][n][32] on the device, and e_ok (may be null; [D] on the device): 0 = the dealer's round-1 data is
// missing, as receivers_rounds takes RoundMasks::e_ok -- the phase-1 intake mask, in full mode joined
// with the decode mask of the dealer's ciphertexts: a MISSING row in round 2.
struct ShardRows {
  const uint32_t *E, *A, *s, *s_prime;
  const uint8_t* e_ok;
};

// Rounds 2-5 of one rank of a dealer-sharded ceremony on its dealers [d0, d0+D) -> decision rows,
// master-key terms, partial final shares.
//
// in.proven (may be null): the rank decides by the PROVEN complaints against its own dealers (ShardProven,
// shard_complaints) -- the stage follows the checks on the stream and gives the qualified mask of the
// partial sums; its df3 goes to verify_rounds as a_ok (the intake mask of the phase-3 broadcasts); in.e1 /
// in.ct are the rank's ciphertexts [D][n][2][8] (full mode: the pairs the round-2 complaints are verified
// against).
void shard_rows(dkg_ctx* ctx, size_t n, size_t t, size_t d0, size_t D, const ShardInput& in, const ShardRows& rows) {
  const uint32_t *Ec = rows.E, *Ac = rows.A, *ds = rows.s, *dsp = rows.s_prime;
  void *d_dec2 = in.dec2, *d_dec4 = in.dec4, *d_A0 = in.A0, *d_partial = in.partial;
  ShardProven* sp = in.proven;
  const uint8_t *e_ok = rows.e_ok, *a_ok = sp ? sp->df3 : nullptr;
  const size_t N = t + 1;
  if (!D) {
    HCK(hipMemsetAsync(d_partial, 0, 32 * n, ctx->stream));
    if (sp) shard_complaints_none(ctx, n, *sp);
    return;
  }
  // the exchanged A_i0 encodings depend only on round 1: encoded on the side stream beside the checks
  // (a latency-bound chain of D lanes that otherwise ends the call), joined before it returns
  const bool side_terms = ctx->ext_A != nullptr;
  if (side_terms) {
    uint32_t* a0 = buf<uint32_t>(ctx, "sh_a0ext", PTB * D);
    HCK(hipEventRecord(ctx->side_fork, ctx->stream));
    HCK(hipStreamWaitEvent(ctx->side, ctx->side_fork, 0));
    dkgk::gather_points(ctx->ext_A, ctx->ext_stride, N, 0, D, a0, D, ctx->side);
    dkgk::encode_points(a0, D, D, (uint32_t*)d_A0, ctx->side);
    HCK(hipEventRecord(ctx->terms_done, ctx->side));
  } else {
    HCK(hipMemcpy2DAsync(d_A0, 32, Ac, 32 * N, 32, D, hipMemcpyDeviceToDevice, ctx->stream));
  }
  // Qualification of a dealer depends only on its own decision row (any REJECT disqualifies,
  // committee.rs:370-398; missing data disqualifies, :331-335), so each rank decides it for its
  // dealers with no exchange -- on the device, queued after the checks (no host round trip)
  uint8_t* rej = buf<uint8_t>(ctx, "sh_rej", D);
  uint8_t* qm = buf<uint8_t>(ctx, "sh_q", D);
  verify_rounds(
      ctx, n, t, D, d0, Ec, Ac, ds, dsp, (uint8_t*)d_dec2, (uint8_t*)d_dec4, nullptr,
      [&] {
        if (sp) return;  // decided after both rounds, from the complaints (below)
        dkgk::row_reject(D, n, (const uint8_t*)d_dec2, rej, ctx->stream);
        dkgk::mask_not_and(D, rej, nullptr, qm, ctx->stream);
      },
      e_ok, a_ok, false);
  if (side_terms) HCK(hipStreamWaitEvent(ctx->stream, ctx->terms_done, 0));
  wait_shares(ctx, ctx->stream);  // shares evaluated on the side stream (round1_device)
  ctx->shares_pending = false;
  // the proven rule: this sits inside the caller's with_binom_ded body, so a rerun with the complete
  // formula reruns the stage on the rerun's tables
  if (sp)
    shard_complaints(ctx, n, t, D, Ec, Ac, (const uint32_t*)in.e1, (const uint32_t*)in.ct, (const uint8_t*)d_dec2, rej,
                     qm, *sp);
  // A dealer accused in round 4 (committee.rs:660-670) has its term replaced after the exchange,
  // once the final parties are known (dkg_ceremony_shard_recon_device): its shares stay here.
  ctx->shard_s = ds;
  ctx->shard_n = n;
  ctx->shard_d0 = d0;
  ctx->shard_D = D;
  dkgk::sum_shares(D, n, ds, qm, (uint32_t*)d_partial, ctx->stream);  // partial of :454-462
}

// The argument prologue of the six dkg_ceremony_shard_*_device entry points; nothing is queued before it
// returns.  `keys`: the host keys the entry point's mode takes (their absence cannot be told from the
// plaintext mode's).  d_partial is written even for a rank without dealers; with dealers the mode's inputs
// and the other three outputs are required.
int shard_args(dkg_ctx* ctx, size_t n, size_t t, size_t d0, size_t d1, const ShardInput& in,
               std::initializer_list<const void*> keys) {
  const int rc = ceremony_args(ctx, n, t, {in.partial});
  if (rc) return rc;
  if (d1 < d0 || d1 > n) return DKG_E_ARG;
  for (const void* k : keys)
    if (!k) return DKG_E_ARG;
  const size_t D = d1 - d0;
  if (D) {
    const bool inputs = in.a      ? in.b && (!in.sk || in.r)
                        : in.sk   ? in.E && in.A && in.e1 && in.ct
                                  : in.E && in.A && in.s && in.s_prime;
    if (!inputs || !in.dec2 || !in.dec4 || !in.A0) return DKG_E_ARG;
  }
  if (const ShardProven* sp = in.proven) {
    if (sp->flag_rows < D || (sp->flag_rows && !sp->d_flags)) return DKG_E_ARG;
    if (!complaint_args_ok(n, sp->C2, sp->accuser2, sp->accused2, {sp->proofs, sp->verdict2}) ||
        !complaint_args_ok(n, sp->C4, sp->accuser4, sp->accused4, {sp->share4, sp->randomness4, sp->verdict4}))
      return DKG_E_ARG;
  }
  return DKG_OK;
}

// Every dkg_ceremony_shard_*_device entry point: one rank's rounds on its dealers [d0, d1).  The timed
// region (ev[0]..ev[1], ms_total) starts after the key uploads and covers the proven staging upload, the
// share stage and the rounds.
//
// Full mode: items, decode masks, MISSING rows and decrypted shares are per dealer, so the hybrid stage
// is shard-local: D dealers' items to all n keys.  With chunk streams it runs on the side stream beside
// the check pipeline's binomial, stepping and recombination, which read no share; the checks wait for
// the decrypted shares (shares_pending / wait_shares), and the ciphertexts' decode mask joins the dealer
// mask there.  Serialised runs (nsub == 1) record the full.* phases.
int shard_ceremony(dkg_ctx* ctx, size_t n, size_t t, size_t d0, size_t d1, const ShardInput& in) {
  const size_t D = d1 - d0, N = t + 1, items = 2 * D * n;
  const bool gen = in.a != nullptr, full = in.sk != nullptr;
  ShardProven* sp = in.proven;
  const uint32_t *dsk = nullptr, *dpk = nullptr;
  if (full) dsk = upload_scalars(ctx, "fm_sk", in.sk, n);
  if (full && gen) {
    uint32_t* p = buf<uint32_t>(ctx, "fm_pk", 32 * n);
    h2d(ctx, p, in.pk, 32 * n);
    dpk = p;
  }
  HCK(hipEventRecord(ctx->ev[0], ctx->stream));
  if (sp) {  // before the side stream forks: it reads the intake mask
    sp->full = full, sp->pk = in.pk;
    shard_proven_upload(ctx, n, d0, D, *sp);
  }
  // the shares the rounds read: generated, received (Scalar::from_bytes semantics: bit 255 cleared,
  // reduced, as upload_scalars) or decrypted
  uint32_t* ds = buf<uint32_t>(ctx, "sh_s", 32 * D * n);
  uint32_t* dsp = buf<uint32_t>(ctx, "sh_sp", 32 * D * n);
  ShardRows rows{(const uint32_t*)in.E, (const uint32_t*)in.A, ds, dsp, sp ? sp->df1 : nullptr};
  // what runs beside the checks on the side stream (one-stream runs: back to back): the generated shares'
  // evaluation, and in full mode the hybrid stage under the fused group check
  const bool side = ctx->nsub > 1 && (!full || ctx->verify_mode == 0);
  hipStream_t hy = side ? ctx->side : ctx->stream;
  SharesScope pending(ctx);  // on an exception the home stream still waits for the side stream's work
  std::optional<ExtScope> ext;
  const uint32_t *e1 = (const uint32_t*)in.e1, *ct = (const uint32_t*)in.ct;
  if (gen) {
    uint32_t* Ec = buf<uint32_t>(ctx, "sh_E", 32 * D * N);
    uint32_t* Ac = buf<uint32_t>(ctx, "sh_A", 32 * D * N);
    // full mode: the dealers' plaintext shares stay apart from what the receivers decrypt
    uint32_t* gs = full ? buf<uint32_t>(ctx, "shg_s", 32 * D * n) : ds;
    uint32_t* gsp = full ? buf<uint32_t>(ctx, "shg_sp", 32 * D * n) : dsp;
    if (D) round1_device(ctx, D, n, t, (const uint32_t*)in.a, (const uint32_t*)in.b, Ec, Ac, gs, gsp, false, side);
    if (D && full) {
      uint32_t* o1 = in.e1_out ? (uint32_t*)in.e1_out : buf<uint32_t>(ctx, "shf_e1", 32 * items);
      uint32_t* oc = in.ct_out ? (uint32_t*)in.ct_out : buf<uint32_t>(ctx, "shf_ct", 32 * items);
      encrypt_device(ctx, D, n, dpk, gs, gsp, (const uint32_t*)in.r, o1, oc, hy, in.pk, true);  // committee.rs:169-172
      e1 = o1, ct = oc;
    }
    ext.emplace(ctx, D, N);
    rows.E = Ec, rows.A = Ac;
  } else if (D && !full) {
    dkgk::reduce_scalars(D * n, (const uint32_t*)in.s, ds, ctx->stream);
    dkgk::reduce_scalars(D * n, (const uint32_t*)in.s_prime, dsp, ctx->stream);
  }
  if (full) {
    uint8_t* iok = buf<uint8_t>(ctx, "shf_iok", items);
    uint8_t* eok = buf<uint8_t>(ctx, "shf_eok", D);
    rows.e_ok = eok;
    if (D) {
      if (side && !gen) {  // round1_device forked the side stream already
        HCK(hipEventRecord(ctx->side_fork, ctx->stream));
        HCK(hipStreamWaitEvent(ctx->side, ctx->side_fork, 0));
      }
      decrypt_device(ctx, D, n, dsk, e1, ct, ds, dsp, iok, eok, hy);  // committee.rs:282-286
      if (sp && sp->df1) dkgk::and_mask(D, sp->df1, eok, hy);  // an absent phase-1 broadcast: a MISSING row as well
      if (side) {
        HCK(hipEventRecord(ctx->shares_done, ctx->side));
        ctx->shares_pending = true;
      }
    }
  }
  with_binom_ded(ctx, [&] {
    shard_rows(ctx, n, t, d0, D, in, rows);
    check_launch(ctx);
    HCK(hipEventRecord(ctx->ev[1], ctx->stream));
    binom_mark_copy(ctx);
    sync(ctx);
  });
  collect_verify_phases(ctx);  // the checks' serialised phases (shard_rows queues no host round trip)
  if (full) phase_collect(ctx, "full", FULL_PHASES, std::size(FULL_PHASES));
  if (sp) shard_proven_verdicts(*sp);
  if (in.ms_total) *in.ms_total = ev_ms(ctx, 0, 1);
  return DKG_OK;
}

int shard_call(dkg_ctx* ctx, size_t n, size_t t, size_t d0, size_t d1, const ShardInput& in,
               std::initializer_list<const void*> keys = {}) {
  return guarded(ctx, [&] {
    const int rc = shard_args(ctx, n, t, d0, d1, in, keys);
    return rc ? rc : shard_ceremony(ctx, n, t, d0, d1, in);
  });
}

extern "C" {

int dkg_ceremony_shard_device(dkg_ctx* ctx, size_t n, size_t t, size_t d0, size_t d1, const void* d_a,
                              const void* d_b, void* d_dec2, void* d_dec4, void* d_A0, void* d_partial,
                              double* ms_total) {
  ShardInput in;
  in.a = d_a, in.b = d_b;
  in.dec2 = d_dec2, in.dec4 = d_dec4, in.A0 = d_A0, in.partial = d_partial, in.ms_total = ms_total;
  return shard_call(ctx, n, t, d0, d1, in);
}

int dkg_ceremony_shard_verify_device(dkg_ctx* ctx, size_t n, size_t t, size_t d0, size_t d1, const void* d_E,
                                     const void* d_A, const void* d_s, const void* d_s_prime, void* d_dec2,
                                     void* d_dec4, void* d_A0, void* d_partial, double* ms_total) {
  ShardInput in;
  in.E = d_E, in.A = d_A, in.s = d_s, in.s_prime = d_s_prime;
  in.dec2 = d_dec2, in.dec4 = d_dec4, in.A0 = d_A0, in.partial = d_partial, in.ms_total = ms_total;
  return shard_call(ctx, n, t, d0, d1, in);
}

// Full mode of the two calls above (dkg_ceremony_run_full_device / dkg_ceremony_verify_full on rows [d0, d1))
int dkg_ceremony_shard_full_device(dkg_ctx* ctx, size_t n, size_t t, size_t d0, size_t d1, const void* d_a,
                                   const void* d_b, const void* d_r, const uint8_t* sk, const uint8_t* pk, void* d_e1,
                                   void* d_ct, void* d_dec2, void* d_dec4, void* d_A0, void* d_partial,
                                   double* ms_total) {
  ShardInput in;
  in.a = d_a, in.b = d_b, in.r = d_r, in.e1_out = d_e1, in.ct_out = d_ct, in.sk = sk, in.pk = pk;
  in.dec2 = d_dec2, in.dec4 = d_dec4, in.A0 = d_A0, in.partial = d_partial, in.ms_total = ms_total;
  return shard_call(ctx, n, t, d0, d1, in, {sk, pk});
}

int dkg_ceremony_shard_verify_full_device(dkg_ctx* ctx, size_t n, size_t t, size_t d0, size_t d1, const void* d_E,
                                          const void* d_A, const void* d_e1, const void* d_ct, const uint8_t* sk,
                                          void* d_dec2, void* d_dec4, void* d_A0, void* d_partial, double* ms_total) {
  ShardInput in;
  in.E = d_E, in.A = d_A, in.e1 = d_e1, in.ct = d_ct, in.sk = sk;
  in.dec2 = d_dec2, in.dec4 = d_dec4, in.A0 = d_A0, in.partial = d_partial, in.ms_total = ms_total;
  return shard_call(ctx, n, t, d0, d1, in, {sk});
}

// dkg_ceremony_shard_verify_device with the reference's rule for the reconstructable set, as
// dkg_ceremony_verify_fetched_proven: round 2 keeps the rejection rule, round 4 is proven.
int dkg_ceremony_shard_verify_proven_device(dkg_ctx* ctx, size_t n, size_t t, size_t d0, size_t d1, const void* d_E,
                                            const void* d_A, const void* d_s, const void* d_s_prime,
                                            const uint8_t* fetched1, const uint8_t* fetched3, size_t C4,
                                            const uint32_t* accuser4, const uint32_t* accused4, const uint8_t* share4,
                                            const uint8_t* randomness4, void* d_dec2, void* d_dec4, void* d_A0,
                                            void* d_partial, size_t flag_rows, void* d_flags, int32_t* verdict4,
                                            double* ms_total) {
  ShardProven sp;
  sp.C4 = C4, sp.accuser4 = accuser4, sp.accused4 = accused4, sp.share4 = share4, sp.randomness4 = randomness4;
  sp.fetched1 = fetched1, sp.fetched3 = fetched3, sp.verdict4 = verdict4;
  sp.flag_rows = flag_rows, sp.d_flags = d_flags;
  ShardInput in;
  in.E = d_E, in.A = d_A, in.s = d_s, in.s_prime = d_s_prime, in.proven = &sp;
  in.dec2 = d_dec2, in.dec4 = d_dec4, in.A0 = d_A0, in.partial = d_partial, in.ms_total = ms_total;
  return shard_call(ctx, n, t, d0, d1, in);
}

// dkg_ceremony_shard_verify_full_device with both rounds decided by the proven complaints, as
// dkg_ceremony_verify_full_proven.
int dkg_ceremony_shard_verify_full_proven_device(dkg_ctx* ctx, size_t n, size_t t, size_t d0, size_t d1,
                                                 const void* d_E, const void* d_A, const void* d_e1, const void* d_ct,
                                                 const uint8_t* sk, const uint8_t* pk, const uint8_t* fetched1,
                                                 const uint8_t* fetched3, size_t C, const uint32_t* accuser,
                                                 const uint32_t* accused, const uint8_t* proofs, size_t C4,
                                                 const uint32_t* accuser4, const uint32_t* accused4,
                                                 const uint8_t* share4, const uint8_t* randomness4, void* d_dec2,
                                                 void* d_dec4, void* d_A0, void* d_partial, size_t flag_rows,
                                                 void* d_flags, void* d_dissent, int32_t* verdict, int32_t* verdict4,
                                                 double* ms_total) {
  ShardProven sp;
  sp.C2 = C, sp.accuser2 = accuser, sp.accused2 = accused, sp.proofs = proofs, sp.verdict2 = verdict;
  sp.C4 = C4, sp.accuser4 = accuser4, sp.accused4 = accused4, sp.share4 = share4, sp.randomness4 = randomness4;
  sp.fetched1 = fetched1, sp.fetched3 = fetched3, sp.verdict4 = verdict4;
  sp.flag_rows = flag_rows, sp.d_flags = d_flags, sp.d_dissent = d_dissent;
  ShardInput in;
  in.E = d_E, in.A = d_A, in.e1 = d_e1, in.ct = d_ct, in.sk = sk, in.pk = pk, in.proven = &sp;
  in.dec2 = d_dec2, in.dec4 = d_dec4, in.A0 = d_A0, in.partial = d_partial, in.ms_total = ms_total;
  return shard_call(ctx, n, t, d0, d1, in, {sk, pk});
}

int dkg_ctx_last_complaint_eval(const dkg_ctx* ctx) { return ctx ? ctx->last_complaint_eval : 0; }

int dkg_ceremony_shard_recon_device(dkg_ctx* ctx, size_t n, size_t t, size_t d0, size_t d1, const uint8_t* qualified,
                                    const uint8_t* reconstruct, const uint8_t* r2_error, const uint8_t* r4_error,
                                    const void* d_s, void* d_terms, int32_t* recovery_error) {
  return guarded(ctx, [&] {
    if (!qualified || !reconstruct || !d_terms || d1 < d0 || d1 > n || dkg_env_check(t, n) != DKG_OK) return DKG_E_ARG;
    const size_t D = d1 - d0;
    // decided from the common outcome alone: the same on every rank, whichever dealers it holds
    const std::vector<uint8_t> disc = disclosing_parties(n, qualified, reconstruct, r2_error, r4_error);
    bool any = false;
    for (size_t i = 0; i < n; i++) any |= reconstruct[i] != 0;
    const bool fails = any && recovery_fails(disc, t);
    if (recovery_error) *recovery_error = fails ? 1 : 0;
    if (fails) return DKG_OK;  // nobody recovers: the caller zeroes the mpk
    std::vector<size_t> rows;
    for (size_t i = 0; i < D; i++) {
      if (reconstruct[d0 + i] && !qualified[d0 + i]) {
        ctx->err = "shard_recon: only qualified members are reconstructed (committee.rs:746-747)";
        return DKG_E_ARG;
      }
      if (reconstruct[d0 + i]) rows.push_back(i);
    }
    if (rows.empty()) return DKG_OK;
    const uint32_t* ds = nullptr;
    if (d_s) {  // received shares: Scalar::from_bytes semantics
      uint32_t* red = buf<uint32_t>(ctx, "shr_s", 32 * D * n);
      dkgk::reduce_scalars(D * n, (const uint32_t*)d_s, red, ctx->stream);
      ds = red;
    } else {
      if (!ctx->shard_s || ctx->shard_n != n || ctx->shard_d0 != d0 || ctx->shard_D != D) {
        ctx->err = "shard_recon: d_s is NULL and the last sharded call on this ctx had other dealers";
        return DKG_E_ARG;
      }
      ds = ctx->shard_s;
    }
    const size_t R = rows.size();
    std::vector<uint8_t> hs(32 * n * R);
    for (size_t r = 0; r < R; r++) d2h(ctx, &hs[32 * n * r], ds + 8 * n * rows[r], 32 * n);
    sync(ctx);
    std::vector<size_t> idx(R);
    for (size_t r = 0; r < R; r++) idx[r] = r;
    std::vector<uint8_t> secrets = recon_secrets(n, disc, hs.data(), idx);
    uint32_t* sec = buf<uint32_t>(ctx, "sh_rsec", 32 * R);
    uint32_t* gsec = buf<uint32_t>(ctx, "sh_rext", PTB * R);
    uint32_t* gc = buf<uint32_t>(ctx, "sh_rcomp", 32 * R);
    h2d(ctx, sec, secrets.data(), secrets.size());
    dkgk::fixed_base(R, sec, ctx->tab_gw, gsec, ctx->stream);  // G::generator() * recovered (:789)
    dkgk::encode_points(gsec, R, R, gc, ctx->stream);
    for (size_t r = 0; r < R; r++)
      HCK(hipMemcpyAsync((uint8_t*)d_terms + 32 * rows[r], gc + 8 * r, 32, hipMemcpyDeviceToDevice, ctx->stream));
    check_launch(ctx);
    sync(ctx);
    return DKG_OK;
  });
}

int dkg_finalise_parties(dkg_ctx* ctx, size_t n, size_t t, const uint8_t* qualified, const uint8_t* reconstruct,
                         const uint8_t* r2_error, const uint8_t* r4_error, const uint8_t* disclosed, const uint8_t* A0,
                         const uint8_t* s, uint8_t* mpk, int32_t* status, int32_t* recovery_index) {
  return guarded(ctx, [&] {
    using namespace dkgh;
    if (!qualified || !reconstruct || !A0 || !s || !mpk || !status) return DKG_E_ARG;
    if (!n) return DKG_OK;
    std::vector<size_t> recon;
    int32_t nq = 0;
    for (size_t i = 0; i < n; i++) {
      if (reconstruct[i] && !qualified[i]) {
        ctx->err = "finalise: only qualified members should be reconstructed (committee.rs:746-747 panics)";
        return DKG_E_ARG;
      }
      nq += qualified[i] != 0;
      if (reconstruct[i]) recon.push_back(i);
    }
    const std::vector<uint8_t> fin = final_parties(n, qualified, reconstruct);
    const bool phase4 = nq - (int32_t)recon.size() <= (int32_t)t;  // committee.rs:673-677
    // S: final parties whose phase-5 disclosures the finalising party fetched (committee.rs:763-775).
    // A party whose Phase1 or Phase3 proceed failed never reaches Phase4::proceed and so never
    // broadcasts a BroadcastPhase5 (:340-347, :567-569, :684), whatever `disclosed` says.
    std::vector<uint8_t> S(n);
    size_t nS = 0;
    for (size_t j = 0; j < n; j++)
      nS += S[j] = fin[j] && (!disclosed || disclosed[j]) && !(r2_error && r2_error[j]) &&
                   !(r4_error && r4_error[j]);
    const Zl zero = zl_from_u64(0), one = zl_from_u64(1);
    std::vector<Zl> lamS, yrows;  // Lagrange coefficients over S; the reconstructed rows' shares
    if (!recon.empty() && !phase4) {
      lamS = lagrange_zero_coeffs(n, S.data());
      yrows.resize(recon.size() * n);
      for (size_t r = 0; r < recon.size(); r++)
        for (size_t j = 0; j < n; j++) yrows[r * n + j] = zl_from_bits(s + 32 * (recon[r] * n + j));
    }
    Zl PS = one;
    for (size_t j = 0; j < n; j++)
      if (S[j]) PS = zl_mul(PS, zl_from_u64(j + 1));
    std::vector<uint8_t> sig(32 * n, 0), ok(n, 0);
    std::vector<Zl> mu(n), inv(n), pre(n);
    for (size_t p = 0; p < n; p++) {
      if (recovery_index) recovery_index[p] = -1;
      if (r2_error && r2_error[p]) { status[p] = DKG_FIN_R2_ERROR; continue; }   // committee.rs:340-347
      if (r4_error && r4_error[p]) { status[p] = DKG_FIN_R4_ERROR; continue; }   // :567-569
      if (phase4) { status[p] = DKG_FIN_PHASE4_ERROR; continue; }                // :673-677
      // the party's own share plus the fetched disclosures of the other final parties (:754-775)
      const size_t cnt = nS + (S[p] ? 0 : 1);
      // finalise walks the dealers in index order (:745-797) and stops at the first of: a
      // reconstructed dealer with fewer than `threshold` (t, not t + 1) points ->
      // InsufficientSharesForRecovery(i) (:779-781); a disqualified dealer other than itself ->
      // the reference PANICS: its committed coefficients were never recorded (committed_shares[i]
      // is set only for itself, :190, and for qualified dealers in Phase3::proceed, :527-530) and
      // :791-794 expect() them.  A disqualified party p adds its own A_p0 (its init state).
      status[p] = DKG_FIN_OK;
      for (size_t i = 0; i < n && status[p] == DKG_FIN_OK; i++) {
        if (reconstruct[i] && cnt < t) status[p] = DKG_FIN_INSUFFICIENT;
        else if (!reconstruct[i] && !qualified[i] && i != p) status[p] = DKG_FIN_PANIC;
        if (status[p] != DKG_FIN_OK && recovery_index) recovery_index[p] = (int32_t)i;
      }
      if (status[p] != DKG_FIN_OK) continue;
      ok[p] = 1;
      if (recon.empty()) continue;
      const std::vector<Zl>* lam = &lamS;
      if (!S[p]) {
        // T = S u {p}: mu_a = lambda^S_a x_p / (x_p - x_a) (a in S), mu_p = prod_{b in S} x_b / (x_b - x_p)
        const Zl xp = zl_from_u64(p + 1);
        std::vector<size_t> as;
        for (size_t a = 0; a < n; a++)
          if (S[a]) as.push_back(a);
        Zl acc = one;  // batch inversion of (x_p - x_a)
        for (size_t k = 0; k < as.size(); k++) {
          pre[k] = acc;
          inv[k] = zl_sub(xp, zl_from_u64(as[k] + 1));
          acc = zl_mul(acc, inv[k]);
        }
        Zl ia = zl_inv(acc);
        for (size_t k = as.size(); k-- > 0;) {
          const Zl d = inv[k];
          inv[k] = zl_mul(ia, pre[k]);
          ia = zl_mul(ia, d);
        }
        Zl prod = one;
        for (size_t a = 0; a < n; a++) mu[a] = zero;
        for (size_t k = 0; k < as.size(); k++) {
          mu[as[k]] = zl_mul(zl_mul(lamS[as[k]], xp), inv[k]);
          prod = zl_mul(prod, zl_sub(zero, inv[k]));  // 1 / (x_b - x_p)
        }
        mu[p] = zl_mul(PS, prod);
        lam = &mu;
      }
      Zl sigma = zero;  // sum over the reconstructed dealers of the recovered secrets (:784-789)
      for (size_t r = 0; r < recon.size(); r++)
        for (size_t a = 0; a < n; a++)
          if (!zl_is_zero((*lam)[a])) sigma = zl_add(sigma, zl_mul((*lam)[a], yrows[r * n + a]));
      zl_to_bytes(&sig[32 * p], sigma);
    }
    memset(mpk, 0, 32 * n);
    size_t nok = 0;
    for (auto v : ok) nok += v;
    if (!nok) return DKG_OK;
    // mpk_p = sum_{final i} A_i0 + G::generator() * sigma_p (:789-795), on the device
    uint32_t* a0c = buf<uint32_t>(ctx, "fp_a0c", 32 * n);
    uint32_t* a0e = buf<uint32_t>(ctx, "fp_a0e", PTB * n);
    uint8_t* a0ok = buf<uint8_t>(ctx, "fp_a0ok", n);
    uint8_t* fm = buf<uint8_t>(ctx, "fp_fin", n);
    uint32_t* hsum = buf<uint32_t>(ctx, "fp_h", PTB);
    uint32_t* hrep = buf<uint32_t>(ctx, "fp_hrep", PTB * n);
    uint32_t* sd = buf<uint32_t>(ctx, "fp_sig", 32 * n);
    uint32_t* ge = buf<uint32_t>(ctx, "fp_ge", PTB * n);
    uint32_t* oc = buf<uint32_t>(ctx, "fp_out", 32 * n);
    h2d(ctx, a0c, A0, 32 * n);
    h2d(ctx, fm, fin.data(), n);
    h2d(ctx, sd, sig.data(), 32 * n);
    dkgk::decode_points(a0c, n, a0e, n, a0ok, ctx->stream);
    dkgk::sum_points(n, a0e, n, fm, hsum, 1, 0, ctx->stream);
    dkgk::gather_points(hsum, 1, 0, 0, n, hrep, n, ctx->stream);
    // a finalising disqualified party (the only disqualified dealer) also adds its own A_p0
    for (size_t p = 0; p < n; p++)
      if (ok[p] && !qualified[p]) dkgk::add_points(1, hrep + p, a0e + p, n, hrep + p, ctx->stream);
    dkgk::fixed_base(n, sd, ctx->tab_gw, ge, ctx->stream);
    dkgk::add_points(n, ge, hrep, n, ge, ctx->stream);
    dkgk::encode_points(ge, n, n, oc, ctx->stream);
    check_launch(ctx);
    std::vector<uint8_t> okh(n), outh(32 * n);
    d2h(ctx, okh.data(), a0ok, n);
    d2h(ctx, outh.data(), oc, 32 * n);
    sync(ctx);
    for (size_t i = 0; i < n; i++)
      if ((fin[i] || (ok[i] && !qualified[i])) && !okh[i]) {
        ctx->err = "finalise: a summed A_0 commitment does not decode";
        return DKG_E_DECODE;
      }
    for (size_t p = 0; p < n; p++)
      if (ok[p]) memcpy(mpk + 32 * p, &outh[32 * p], 32);
    return DKG_OK;
  });
}

int dkg_scalar_sum_device(dkg_ctx* ctx, size_t rows, size_t n, const void* d_in, const void* d_mask, void* d_out) {
  return guarded(ctx, [&] {
    const uint8_t* mask = (const uint8_t*)d_mask;
    if (!mask) {
      uint8_t* ones = buf<uint8_t>(ctx, "ss_ones", rows);
      HCK(hipMemsetAsync(ones, 1, rows, ctx->stream));
      mask = ones;
    }
    dkgk::sum_shares(rows, n, (const uint32_t*)d_in, mask, (uint32_t*)d_out, ctx->stream);
    check_launch(ctx);
    sync(ctx);
    return DKG_OK;
  });
}

int dkg_point_sum_device(dkg_ctx* ctx, size_t count, const void* d_points, const void* d_mask, void* d_out) {
  return guarded(ctx, [&] {
    uint32_t* ext = buf<uint32_t>(ctx, "ps_ext", PTB * count);
    uint8_t* ok = buf<uint8_t>(ctx, "ps_ok", count);
    uint32_t* sum = buf<uint32_t>(ctx, "ps_sum", PTB);
    dkgk::decode_points((const uint32_t*)d_points, count, ext, count, ok, ctx->stream);
    dkgk::sum_points(count, ext, count, (const uint8_t*)d_mask, sum, 1, 0, ctx->stream);
    dkgk::encode_points(sum, 1, 1, (uint32_t*)d_out, ctx->stream);
    check_launch(ctx);
    std::vector<uint8_t> okh(count), mh(count, 1);
    d2h(ctx, okh.data(), ok, count);
    if (d_mask) d2h(ctx, mh.data(), d_mask, count);
    sync(ctx);
    for (size_t c = 0; c < count; c++)
      if (mh[c] && !okh[c]) {
        ctx->err = "point_sum: a selected point does not decode";
        return DKG_E_DECODE;
      }
    return DKG_OK;
  });
}

void dkg_shard_range(size_t n, size_t world_size, size_t rank, size_t* d0, size_t* d1) {
  const size_t ws = world_size ? world_size : 1;
  if (d0) *d0 = rank < ws ? (rank * n) / ws : n;
  if (d1) *d1 = rank < ws ? ((rank + 1) * n) / ws : n;
}

size_t dkg_shard_rows(size_t n, size_t world_size) {
  size_t R = 0;
  for (size_t r = 0; r < world_size; r++) R = std::max(R, ((r + 1) * n) / world_size - (r * n) / world_size);
  return R;
}

}  // extern "C"

// The combine of the sharded run from the gathered rank blocks: `dense` materialises them as the
// [n][n] matrices (compacted bytes or unpacked bitmaps), then the single-GPU drivers' outcome code.
template <typename F>
int shard_combine(dkg_ctx* ctx, size_t n, size_t t, void* d_dec2, void* d_dec4, dkg_shard_outcome* out, F&& dense) {
  uint8_t* dec2 = d_dec2 ? (uint8_t*)d_dec2 : buf<uint8_t>(ctx, "sc.dec2", n * n);
  uint8_t* dec4 = d_dec4 ? (uint8_t*)d_dec4 : buf<uint8_t>(ctx, "sc.dec4", n * n);
  uint8_t* qmask = buf<uint8_t>(ctx, "sc.qmask", n);
  dense(dec2, dec4);
  // both rounds' device halves, then one copy-back (pinned) and one sync
  uint8_t* rej2 = buf<uint8_t>(ctx, "sc.rej2", n);
  int32_t* cnt = buf<int32_t>(ctx, "sc.cnt", 4 * n);
  uint8_t* rej4 = buf<uint8_t>(ctx, "sc.rej4", n);
  uint8_t* r4d = buf<uint8_t>(ctx, "sc.r4err", n);
  round2_device(ctx, 1, n, dec2, qmask, rej2, cnt);
  round4_device(ctx, 1, n, t, dec4, qmask, rej4, r4d);
  check_launch(ctx);
  uint8_t* h = hbuf<uint8_t>(ctx, "sc.out", 7 * n);  // rej2 | rej4 | r4err | cnt
  d2h(ctx, h, rej2, n);
  d2h(ctx, h + n, rej4, n);
  d2h(ctx, h + 2 * n, r4d, n);
  d2h(ctx, h + 3 * n, cnt, 4 * n);
  sync(ctx);
  std::vector<uint8_t> q(h, h + n), r2e(n), recon(h + n, h + 2 * n), r4e(h + 2 * n, h + 3 * n);
  std::vector<int32_t> c(n);
  memcpy(c.data(), h + 3 * n, 4 * n);
  round2_host(n, t, q.data(), c.data(), r2e.data());
  round4_host(n, q.data(), recon.data());
  int32_t nq = 0, nr = 0;
  for (size_t i = 0; i < n; i++) {
    nq += q[i];
    nr += recon[i];
  }
  if (out->qualified) memcpy(out->qualified, q.data(), n);
  if (out->complaints2) memcpy(out->complaints2, c.data(), 4 * n);
  if (out->r2_error) memcpy(out->r2_error, r2e.data(), n);
  if (out->reconstruct) memcpy(out->reconstruct, recon.data(), n);
  if (out->r4_error) memcpy(out->r4_error, r4e.data(), n);
  out->n_qualified = nq;
  out->phase4_error = nq - nr <= (int32_t)t;  // committee.rs:673-677
  return DKG_OK;
}

extern "C" {

int dkg_shard_combine_device(dkg_ctx* ctx, size_t n, size_t t, size_t world_size, const void* d_dec2_g,
                             const void* d_dec4_g, void* d_dec2, void* d_dec4, dkg_shard_outcome* out) {
  return guarded(ctx, [&] {
    if (!out || !d_dec2_g || !d_dec4_g || !world_size || world_size > n || dkg_env_check(t, n) != DKG_OK)
      return DKG_E_ARG;
    const size_t R = dkg_shard_rows(n, world_size);
    return shard_combine(ctx, n, t, d_dec2, d_dec4, out, [&](uint8_t* dec2, uint8_t* dec4) {
      dkgk::compact_ranks(n, world_size, R, n, d_dec2_g, dec2, ctx->stream);
      dkgk::compact_ranks(n, world_size, R, n, d_dec4_g, dec4, ctx->stream);
    });
  });
}

size_t dkg_packed_row_words(size_t n) { return (n + 31) / 32 + 1; }

int dkg_fixed_base_windows(void) { return dkgk::fixed_base_windows(); }
int dkg_key_comb_windows(void) { return dkgk::key_comb_windows(); }

int dkg_ctx_set_key_comb(dkg_ctx* ctx, int mode) {
  if (!ctx || mode < 0 || mode > 2) return DKG_E_ARG;
  ctx->key_comb = mode;
  return DKG_OK;
}
int dkg_ctx_last_key_comb(const dkg_ctx* ctx) { return ctx ? ctx->last_key_comb : 0; }

int dkg_ctx_set_seat_deal(dkg_ctx* ctx, int mode) {
  if (!ctx || mode < 0 || mode > 2) return DKG_E_ARG;
  ctx->seat_deal = mode;
  return DKG_OK;
}
int dkg_ctx_last_seat_deal(const dkg_ctx* ctx) { return ctx ? ctx->last_seat_deal : 0; }

int dkg_ctx_set_seat_eval(dkg_ctx* ctx, int mode, int chunk) {
  if (!ctx || mode < 0 || mode > 2 || chunk < 0 || (mode != 2 && chunk != 0)) return DKG_E_ARG;
  ctx->seat_eval = mode;
  ctx->seat_eval_chunk = chunk;
  return DKG_OK;
}
int dkg_ctx_last_seat_eval(const dkg_ctx* ctx, int* chunk) {
  if (chunk) *chunk = ctx ? ctx->last_seat_eval_chunk : 0;
  return ctx ? ctx->last_seat_eval : 0;
}

int dkg_ctx_set_comb_build(dkg_ctx* ctx, int mode) {
  if (!ctx || mode < 0 || mode > 2) return DKG_E_ARG;
  ctx->comb_build = mode;
  // tables of the other builder must not pass for this one's: the caller base's comb and the member
  // keys' radix-2^BITS combs are rebuilt at their next use
  ctx->fb_valid = false;
  ctx->key_tabs_pk.clear();
  return DKG_OK;
}
int dkg_ctx_last_comb_build(const dkg_ctx* ctx) { return ctx ? ctx->last_comb_build : 0; }
double dkg_ctx_last_comb_build_ms(const dkg_ctx* ctx) {
  if (!ctx || !ctx->last_comb_build) return 0.0;
  float ms = 0;
  if (hipEventSynchronize(ctx->cb_ev[1]) != hipSuccess) return 0.0;
  if (hipEventElapsedTime(&ms, ctx->cb_ev[0], ctx->cb_ev[1]) != hipSuccess) return 0.0;
  return ms;
}

int dkg_comb_geometry(int kind, int* bits, int* windows, uint32_t* entries, uint32_t* chunk) {
  return dkgk::comb_geometry(kind, bits, windows, entries, chunk) ? DKG_OK : DKG_E_ARG;
}

int dkg_comb_entries(dkg_ctx* ctx, int kind, const uint8_t base[32], int window, uint32_t first, uint32_t count,
                     uint8_t* out) {
  return guarded(ctx, [&] {
    int windows = 0;
    uint32_t entries = 0;
    if (!dkgk::comb_geometry(kind, nullptr, &windows, &entries, nullptr)) return DKG_E_ARG;
    if (window < 0 || window >= windows || first > entries || count > entries - first) {
      ctx->err = "comb_entries: window or range outside the comb's geometry";
      return DKG_E_ARG;
    }
    if (count == 0) return DKG_OK;
    if (!out) return DKG_E_ARG;
    uint32_t* comp = buf<uint32_t>(ctx, "comb_in", 32);
    uint32_t* ext = buf<uint32_t>(ctx, "comb_ext", PTB);
    uint8_t* okd = buf<uint8_t>(ctx, "comb_ok", 1);
    h2d(ctx, comp, base ? base : BASEPOINT, 32);
    dkgk::decode_points(comp, 1, ext, 1, okd, ctx->stream);
    check_launch(ctx);
    uint8_t v = 0;
    d2h(ctx, &v, okd, 1);
    sync(ctx);
    if (!v) {
      ctx->err = "comb_entries: base point failed to decode";
      return DKG_E_DECODE;
    }
    // always a fresh build: kind 0 into the caller base's buffer (470 MB; its cached comb is given up)
    uint32_t* tab;
    if (kind == 0) {
      tab = buf<uint32_t>(ctx, "fb_tabw", COMBW_BYTES);
      ctx->fb_valid = false;
    } else {
      tab = buf<uint32_t>(ctx, "ce.tab", 4 * dkgk::key_comb_words());
    }
    build_combs(ctx, kind, ext, 1, 0, tab, ctx->stream, 1);
    uint32_t* ob = buf<uint32_t>(ctx, "ce.out", (size_t)96 * count);
    dkgk::comb_entries_bytes(kind, tab, window, first, count, ob, ctx->stream);
    check_launch(ctx);
    d2h(ctx, out, ob, (size_t)96 * count);
    sync(ctx);
    return DKG_OK;
  });
}

// Which comb of the recipient keys serves K = pk_q r for `keys` keys with items_per_key items each (a
// shard of D dealers: 2 D): the smaller of build (unless that kind's tables are cached) + multiplication.
// The constants are the "fit" of profiles/shard_full_time.json (tools/shard_full_time.py on one MI355X):
//   build = floor + per key, a two-point fit through the cold - cached difference of the whole call's
//           device time at n = 64 (all dealers) and n = 1024 (the 8-way shard, where the side stream
//           hides least of it): radix 2^10 957 us + 71.8 us per key (k_build_combw<10>; 74.8 us per
//           key in profiles/r06_rocprof_full_summary.txt), radix 16 558 us + 0.79 us per key
//           (k_benc_tab: one wave's chain of 224 doublings and 64 additions is the floor; 0.07 us per
//           key at the batches' 640,000 keys, profiles/batch_full_time.json).  Both builds have a
//           floor, so both kinds carry one -- with a floor on radix 16 alone, ten cold keys would take
//           the radix-2^10 tables, which at n = 64 measure 7.9 ms against 3.0 ms;
//   mul   = the serialised full.enc_mul phase per item (e1 = g r and K = pk r together, so the two
//           kinds' figures differ by the K products alone): 1.63 ns (k_enc_mul) and 2.81 ns
//           (k_fixed_base + k_benc_mul) at n = 1024, 2,097,152 items.
// With them a cold key set takes radix 16 at every ceremony size (its build is cheaper in floor and
// per key; the dearer products would outweigh that only past ~60,000 items per key), and a cached
// radix-2^10 set is kept.
constexpr double KC10_FLOOR_US = 957.0, KC10_BUILD_US = 71.8, KC10_MUL_NS = 1.63;
constexpr double KC16_FLOOR_US = 558.0, KC16_BUILD_US = 0.79, KC16_MUL_NS = 2.81;

void dkg_key_comb_constants(double c[6]) {
  if (!c) return;
  c[0] = KC10_FLOOR_US, c[1] = KC10_BUILD_US, c[2] = KC10_MUL_NS;
  c[3] = KC16_FLOOR_US, c[4] = KC16_BUILD_US, c[5] = KC16_MUL_NS;
}

int dkg_key_comb_choice(size_t keys, size_t items_per_key, int cached10, int cached16) {
  const double k = (double)keys, work = k * (double)items_per_key;
  const double c10 = (cached10 ? 0.0 : (KC10_FLOOR_US + KC10_BUILD_US * k) * 1e3) + KC10_MUL_NS * work;  // ns
  const double c16 = (cached16 ? 0.0 : (KC16_FLOOR_US + KC16_BUILD_US * k) * 1e3) + KC16_MUL_NS * work;
  return c16 < c10 ? 2 : 1;
}

int dkg_decisions_pack_device(dkg_ctx* ctx, size_t rows, size_t nvalid, size_t n, size_t d0, const void* d_dec,
                              void* d_packed) {
  return guarded(ctx, [&] {
    if (!n || nvalid > rows || (nvalid && !d_dec) || (rows && !d_packed) || d0 + nvalid > n) return DKG_E_ARG;
    if (!rows) return DKG_OK;
    uint32_t* err = buf<uint32_t>(ctx, "pk.err", 4);
    HCK(hipMemsetAsync(err, 0, 4, ctx->stream));
    dkgk::pack_rows(rows, nvalid, n, d0, (const uint8_t*)d_dec, (uint32_t*)d_packed, err, ctx->stream);
    check_launch(ctx);
    uint32_t e = 0;
    d2h(ctx, &e, err, 4);
    sync(ctx);
    if (e) {
      ctx->err = "decisions_pack: a row holds values the packed encoding cannot carry";
      return DKG_E_ARG;
    }
    return DKG_OK;
  });
}

int dkg_shard_combine_packed_device(dkg_ctx* ctx, size_t n, size_t t, size_t world_size, const void* d_pack2_g,
                                    const void* d_pack4_g, void* d_dec2, void* d_dec4, dkg_shard_outcome* out) {
  return guarded(ctx, [&] {
    if (!out || !d_pack2_g || !d_pack4_g || !world_size || world_size > n || dkg_env_check(t, n) != DKG_OK)
      return DKG_E_ARG;
    const size_t R = dkg_shard_rows(n, world_size);
    return shard_combine(ctx, n, t, d_dec2, d_dec4, out, [&](uint8_t* dec2, uint8_t* dec4) {
      dkgk::unpack_ranks(n, world_size, R, (const uint32_t*)d_pack2_g, dec2, ctx->stream);
      dkgk::unpack_ranks(n, world_size, R, (const uint32_t*)d_pack4_g, dec4, ctx->stream);
    });
  });
}

// The combine of the sharded proven calls: dkg_shard_combine_packed_device's, except that the two sets
// follow the ranks' flag words (round2_device's cmask path and the proven4 mask, as receivers_rounds_once
// takes them), plus the sum of the dissent partials and the finalising parties' common outcome.
int dkg_shard_combine_proven_device(dkg_ctx* ctx, size_t n, size_t t, size_t world_size, const void* d_pack2_g,
                                    const void* d_pack4_g, const void* d_flags_g, const void* d_dissent_g, int full,
                                    void* d_dec2, void* d_dec4, dkg_shard_outcome* out, int32_t* dissent,
                                    int32_t* finalise_status, int32_t* recovery_index) {
  return guarded(ctx, [&] {
    if (!out || !d_pack2_g || !d_pack4_g || !d_flags_g || !world_size || world_size > n ||
        dkg_env_check(t, n) != DKG_OK || (dissent && !d_dissent_g))
      return DKG_E_ARG;
    const size_t R = dkg_shard_rows(n, world_size);
    hipStream_t st = ctx->stream;
    uint8_t* dec2 = d_dec2 ? (uint8_t*)d_dec2 : buf<uint8_t>(ctx, "sc.dec2", n * n);
    uint8_t* dec4 = d_dec4 ? (uint8_t*)d_dec4 : buf<uint8_t>(ctx, "sc.dec4", n * n);
    uint8_t* qmask = buf<uint8_t>(ctx, "sc.qmask", n);
    dkgk::unpack_ranks(n, world_size, R, (const uint32_t*)d_pack2_g, dec2, st);
    dkgk::unpack_ranks(n, world_size, R, (const uint32_t*)d_pack4_g, dec4, st);
    uint32_t* flags = buf<uint32_t>(ctx, "scp.flags", 4 * n);
    uint8_t* masks = buf<uint8_t>(ctx, "scp.masks", 3 * n);  // cmask | proven4 | a_ok
    dkgk::compact_ranks(n, world_size, R, 4, d_flags_g, flags, st);
    dkgk::flag_masks(n, flags, masks, masks + n, masks + 2 * n, st);
    uint8_t* rej2 = buf<uint8_t>(ctx, "sc.rej2", n);
    int32_t* cnt = buf<int32_t>(ctx, "sc.cnt", 4 * n);
    uint8_t* rej4 = buf<uint8_t>(ctx, "sc.rej4", n);
    uint8_t* r4d = buf<uint8_t>(ctx, "sc.r4err", n);
    round2_device(ctx, 1, n, dec2, qmask, rej2, cnt, full ? masks : nullptr);
    round4_device(ctx, 1, n, t, dec4, qmask, rej4, r4d);
    int32_t* dsum = buf<int32_t>(ctx, "scp.dissent", 4 * n);
    if (dissent) dkgk::sum_partials_i32(world_size, n, (const int32_t*)d_dissent_g, dsum, st);
    check_launch(ctx);
    uint8_t* h = hbuf<uint8_t>(ctx, "scp.out", 12 * n);  // rej2 | proven4 | r4err | a_ok | cnt | dissent
    d2h(ctx, h, rej2, n);
    d2h(ctx, h + n, masks + n, n);
    d2h(ctx, h + 2 * n, r4d, n);
    d2h(ctx, h + 3 * n, masks + 2 * n, n);
    d2h(ctx, h + 4 * n, cnt, 4 * n);
    if (dissent) d2h(ctx, h + 8 * n, dsum, 4 * n);
    sync(ctx);
    std::vector<uint8_t> q(h, h + n), r2e(n), recon(h + n, h + 2 * n), r4e(h + 2 * n, h + 3 * n);
    std::vector<int32_t> c(n);
    memcpy(c.data(), h + 4 * n, 4 * n);
    round2_host(n, t, q.data(), c.data(), r2e.data());
    round4_host(n, q.data(), recon.data());  // reconstruct = qualified && some complaint holds (:639, :664-669)
    int32_t nq = 0, nr = 0;
    for (size_t i = 0; i < n; i++) {
      nq += q[i];
      nr += recon[i];
    }
    if (out->qualified) memcpy(out->qualified, q.data(), n);
    if (out->complaints2) memcpy(out->complaints2, c.data(), 4 * n);
    if (out->r2_error) memcpy(out->r2_error, r2e.data(), n);
    if (out->reconstruct) memcpy(out->reconstruct, recon.data(), n);
    if (out->r4_error) memcpy(out->r4_error, r4e.data(), n);
    out->n_qualified = nq;
    out->phase4_error = nq - nr <= (int32_t)t;  // committee.rs:673-677
    if (dissent) memcpy(dissent, h + 8 * n, 4 * n);
    int32_t index = -1;
    const int32_t status = finalise_outcome(n, t, q.data(), recon.data(), r2e.data(), r4e.data(), h + 3 * n,
                                            out->phase4_error != 0, &index);
    if (finalise_status) *finalise_status = status;
    if (recovery_index) *recovery_index = index;
    return DKG_OK;
  });
}

int dkg_shard_finalise_device(dkg_ctx* ctx, size_t n, size_t t, size_t world_size, const void* d_terms_g,
                              const void* d_partials_g, const uint8_t* qualified, int phase4_error,
                              void* d_final_share, void* d_public_share, uint8_t* mpk) {
  return guarded(ctx, [&] {
    if (!d_terms_g || !d_partials_g || !qualified || !d_final_share || !mpk || !world_size || world_size > n ||
        dkg_env_check(t, n) != DKG_OK)
      return DKG_E_ARG;
    int rc = need_env(ctx);
    if (rc) return rc;
    const size_t R = dkg_shard_rows(n, world_size);
    // round 3 (committee.rs:454-467): s_j = sum over the ranks' partials, g * s_j
    uint8_t* ones = buf<uint8_t>(ctx, "sf.ones", world_size);
    HCK(hipMemsetAsync(ones, 1, world_size, ctx->stream));
    dkgk::sum_shares(world_size, n, (const uint32_t*)d_partials_g, ones, (uint32_t*)d_final_share, ctx->stream);
    if (d_public_share) {
      // the public shares run on the side stream beside the mpk's decode/sum/encode (both chains
      // are a few latency-bound launches of n threads); joined below before anything is read
      uint32_t* pub = buf<uint32_t>(ctx, "sf.pub", PTB * n);
      HCK(hipEventRecord(ctx->side_fork, ctx->stream));
      HCK(hipStreamWaitEvent(ctx->side, ctx->side_fork, 0));
      dkgk::fixed_base(n, (const uint32_t*)d_final_share, ctx->tab_gw, pub, ctx->side);
      dkgk::encode_points(pub, n, n, (uint32_t*)d_public_share, ctx->side);
      HCK(hipEventRecord(ctx->pub_done, ctx->side));
    }
    auto join_public = [&] {
      if (d_public_share) HCK(hipStreamWaitEvent(ctx->stream, ctx->pub_done, 0));
    };
    memset(mpk, 0, 32);
    if (!phase4_error) {
      // finalise (committee.rs:790-795): the qualified dealers' terms -- A_i0 for the final parties,
      // g * a_i0 recovered over the final parties for the reconstructed ones
      uint32_t* terms = buf<uint32_t>(ctx, "sf.terms", 32 * n);
      uint32_t* ext = buf<uint32_t>(ctx, "sf.ext", PTB * n);
      uint8_t* ok = buf<uint8_t>(ctx, "sf.ok", n);
      uint8_t* qm = buf<uint8_t>(ctx, "sf.q", n);
      uint32_t* sum = buf<uint32_t>(ctx, "sf.sum", PTB);
      uint32_t* mc = buf<uint32_t>(ctx, "sf.mpk", 32);
      // small host transfers through pinned staging ([qualified | ok | mpk]): no pageable bounce
      uint8_t* h = hbuf<uint8_t>(ctx, "sf.host", 2 * n + 32);
      memcpy(h, qualified, n);
      dkgk::compact_ranks(n, world_size, R, 32, d_terms_g, terms, ctx->stream);
      h2d(ctx, qm, h, n);
      dkgk::decode_points(terms, n, ext, n, ok, ctx->stream);
      dkgk::sum_points(n, ext, n, qm, sum, 1, 0, ctx->stream);
      dkgk::encode_points(sum, 1, 1, mc, ctx->stream);
      join_public();
      check_launch(ctx);
      d2h(ctx, h + n, ok, n);
      d2h(ctx, h + 2 * n, mc, 32);
      sync(ctx);
      for (size_t i = 0; i < n; i++)
        if (qualified[i] && !h[n + i]) {
          ctx->err = "shard_finalise: a qualified dealer's master-key term does not decode";
          return DKG_E_DECODE;
        }
      memcpy(mpk, h + 2 * n, 32);
      return DKG_OK;  // synced above, the public shares joined
    }
    join_public();
    check_launch(ctx);
    sync(ctx);
    return DKG_OK;
  });
}

int dkg_ceremony_batch_device(dkg_ctx* ctx, size_t B, size_t n, size_t t, const void* d_a, const void* d_b,
                              dkg_batch_out* out) {
  return guarded(ctx, [&] {
    const int rc = ceremony_args(ctx, n, t, {out});
    if (rc || !B) return rc;
    const size_t N = t + 1, V = B * n;
    HCK(hipEventRecord(ctx->ev[0], ctx->stream));
    uint32_t* Ec = buf<uint32_t>(ctx, "bat_E", 32 * V * N);
    uint32_t* Ac = buf<uint32_t>(ctx, "bat_A", 32 * V * N);
    uint32_t* ds = buf<uint32_t>(ctx, "bat_s", 32 * V * n);
    uint32_t* dsp = buf<uint32_t>(ctx, "bat_sp", 32 * V * n);
    BatchRound1 r1(ctx, V, n, t, (const uint32_t*)d_a, (const uint32_t*)d_b, ds, dsp);
    HCK(hipEventRecord(ctx->ev[1], ctx->stream));
    // round 1 in extended form for the verification: from the deferred commitments' position-major
    // table (BatchRound1), else from round1_device's E/A arrays
    std::unique_ptr<ExtScope> ext(r1.deferred() ? nullptr : new ExtScope(ctx, V, N));
    batch_receivers(ctx, B, n, t, Ec, Ac, ds, dsp, out);
    batch_times(ctx, out, true);
    return DKG_OK;
  });
}

int dkg_ceremony_batch_verify(dkg_ctx* ctx, size_t B, size_t n, size_t t, const uint8_t* E, const uint8_t* A,
                              const uint8_t* s, const uint8_t* s_prime, dkg_batch_out* out) {
  return guarded(ctx, [&] {
    const int rc = ceremony_args(ctx, n, t, {out, E, A, s, s_prime});
    if (rc || !B) return rc;
    BatchInput in;
    in.E = E, in.A = A, in.s = s, in.s_prime = s_prime;
    return verify_batch(ctx, B, n, t, in, out);
  });
}

int dkg_dealer_coeffs_device(dkg_ctx* ctx, const uint8_t master[32], uint32_t ceremony0, size_t B, size_t d0,
                             size_t D, size_t t, void* d_a, void* d_b) {
  return guarded(ctx, [&] {
    if (!master || !d_a || !d_b) return DKG_E_ARG;
    const size_t rows = B * D;
    if (!rows) return DKG_OK;
    uint32_t* m = buf<uint32_t>(ctx, "sg_master", 32);
    uint32_t* seeds = buf<uint32_t>(ctx, "sg_seeds", 32 * rows);
    h2d(ctx, m, master, 32);
    dkgk::dealer_coeffs(rows, D, d0, ceremony0, m, t + 1, seeds, (uint32_t*)d_a, (uint32_t*)d_b, ctx->stream);
    check_launch(ctx);
    sync(ctx);
    return DKG_OK;
  });
}

int dkg_member_keys(dkg_ctx* ctx, const uint8_t master[32], uint32_t ceremony, size_t n, uint8_t* sk_out,
                    uint8_t* pk_out) {
  return guarded(ctx, [&] {
    if (!master || !sk_out || !pk_out) return DKG_E_ARG;
    if (!n) return DKG_OK;
    static const char tag[] = "dkg-amd/v1/member";
    std::vector<uint8_t> sk(32 * n), pk(32 * n);
    for (size_t j = 0; j < n; j++) {  // MemberCommunicationKey::new (procedure_keys.rs:72-76), seeded
      uint8_t msg[sizeof tag - 1 + 40], seed[32], st[64];
      memcpy(msg, tag, sizeof tag - 1);
      memcpy(msg + sizeof tag - 1, master, 32);
      for (int k = 0; k < 4; k++) {
        msg[sizeof tag - 1 + 32 + k] = (uint8_t)(ceremony >> (8 * k));
        msg[sizeof tag - 1 + 36 + k] = (uint8_t)((uint32_t)j >> (8 * k));
      }
      dkgh::blake2b(seed, 32, msg, sizeof msg);
      dkgh::chacha20(seed, 0, st, 64);
      dkgh::zl_to_bytes(&sk[32 * j], dkgh::zl_from_bytes_wide(st, 64));
    }
    uint32_t* dsk = buf<uint32_t>(ctx, "mk_sk", 32 * n);
    uint32_t* dpe = buf<uint32_t>(ctx, "mk_pk_ext", PTB * n);
    uint32_t* dpc = buf<uint32_t>(ctx, "mk_pk", 32 * n);
    h2d(ctx, dsk, sk.data(), 32 * n);
    dkgk::fixed_base(n, dsk, ctx->tab_gw, dpe, ctx->stream);  // to_public (procedure_keys.rs:78-82)
    dkgk::encode_points(dpe, n, n, dpc, ctx->stream);
    check_launch(ctx);
    d2h(ctx, pk.data(), dpc, 32 * n);
    sync(ctx);
    // committee.rs:134-135: ordered_pks.sort() by the byte order of procedure_keys.rs:26-40
    std::vector<size_t> order(n);
    for (size_t j = 0; j < n; j++) order[j] = j;
    std::sort(order.begin(), order.end(),
              [&](size_t a, size_t b) { return memcmp(&pk[32 * a], &pk[32 * b], 32) < 0; });
    for (size_t q = 0; q < n; q++) {
      memcpy(sk_out + 32 * q, &sk[32 * order[q]], 32);
      memcpy(pk_out + 32 * q, &pk[32 * order[q]], 32);
    }
    return DKG_OK;
  });
}

int dkg_enc_randomness(const uint8_t master[32], uint32_t ceremony, size_t d0, size_t D, size_t n, size_t t,
                       uint8_t* r) {
  if (!master || !r) return DKG_E_ARG;
  static const char tag[] = "dkg-amd/v1/dealer";
  std::vector<uint8_t> stream(2 * n * 64);
  for (size_t i = 0; i < D; i++) {
    uint8_t msg[sizeof tag - 1 + 40], seed[32];
    memcpy(msg, tag, sizeof tag - 1);
    memcpy(msg + sizeof tag - 1, master, 32);
    const uint32_t dealer = (uint32_t)(d0 + i);
    for (int k = 0; k < 4; k++) {
      msg[sizeof tag - 1 + 32 + k] = (uint8_t)(ceremony >> (8 * k));
      msg[sizeof tag - 1 + 36 + k] = (uint8_t)(dealer >> (8 * k));
    }
    dkgh::blake2b(seed, 32, msg, sizeof msg);
    dkgh::chacha20(seed, 2 * (t + 1), stream.data(), stream.size());  // after the 2(t+1) coefficients
    for (size_t q = 0; q < 2 * n; q++)
      dkgh::zl_to_bytes(r + 32 * (i * 2 * n + q), dkgh::zl_from_bytes_wide(&stream[64 * q], 64));
  }
  return DKG_OK;
}

int dkg_enc_randomness_device(dkg_ctx* ctx, const uint8_t master[32], uint32_t ceremony0, size_t B, size_t d0,
                              size_t D, size_t n, size_t t, void* d_r) {
  return guarded(ctx, [&] {
    if (!master || !d_r) return DKG_E_ARG;
    const size_t rows = B * D;
    if (!rows || !n) return DKG_OK;
    uint32_t* m = buf<uint32_t>(ctx, "sg_master", 32);
    uint32_t* seeds = buf<uint32_t>(ctx, "sg_seeds", 32 * rows);
    h2d(ctx, m, master, 32);
    dkgk::dealer_seeds(rows, D, d0, ceremony0, m, seeds, ctx->stream);
    dkgk::enc_randomness(rows, n, t + 1, seeds, (uint32_t*)d_r, ctx->stream);
    check_launch(ctx);
    sync(ctx);
    return DKG_OK;
  });
}

int dkg_encrypt_shares(dkg_ctx* ctx, size_t D, size_t n, const uint8_t* pk, const uint8_t* s, const uint8_t* s_prime,
                       const uint8_t* r, uint8_t* e1, uint8_t* ct) {
  return guarded(ctx, [&] {
    if (!pk || !s || !s_prime || !r || !e1 || !ct) return DKG_E_ARG;
    if (!D || !n) return DKG_OK;
    const size_t items = 2 * D * n;
    uint32_t* dpk = buf<uint32_t>(ctx, "hx_pk", 32 * n);
    h2d(ctx, dpk, pk, 32 * n);
    std::vector<uint8_t> ok(n);
    uint32_t* ds = upload_scalars(ctx, "hx_s", s, D * n);
    uint32_t* dsp = upload_scalars(ctx, "hx_sp", s_prime, D * n);
    uint32_t* dr = upload_scalars(ctx, "hx_r", r, items);
    uint32_t* de1 = buf<uint32_t>(ctx, "hx_e1", 32 * items);
    uint32_t* dct = buf<uint32_t>(ctx, "hx_ct", 32 * items);
    // the host keys: a repeated key set reuses its decoded points and combs (1.7 MB per key)
    const uint8_t* pk_ok = encrypt_device(ctx, D, n, dpk, ds, dsp, dr, de1, dct, nullptr, pk);
    d2h(ctx, ok.data(), pk_ok, n);
    d2h(ctx, e1, de1, 32 * items);
    d2h(ctx, ct, dct, 32 * items);
    sync(ctx);
    for (auto v : ok)
      if (!v) {
        ctx->err = "encrypt_shares: a recipient public key does not decode";
        return DKG_E_DECODE;
      }
    return DKG_OK;
  });
}

int dkg_decrypt_shares(dkg_ctx* ctx, size_t D, size_t n, const uint8_t* sk, const uint8_t* e1, const uint8_t* ct,
                       uint8_t* s, uint8_t* s_prime, uint8_t* ok) {
  return guarded(ctx, [&] {
    if (!sk || !e1 || !ct || !s || !s_prime) return DKG_E_ARG;
    if (!D || !n) return DKG_OK;
    const size_t items = 2 * D * n;
    uint32_t* dsk = upload_scalars(ctx, "hx_sk", sk, n);
    uint32_t* de1 = buf<uint32_t>(ctx, "hx_e1", 32 * items);
    uint32_t* dct = buf<uint32_t>(ctx, "hx_ct", 32 * items);
    h2d(ctx, de1, e1, 32 * items);
    h2d(ctx, dct, ct, 32 * items);
    uint32_t* ds = buf<uint32_t>(ctx, "hx_s", 32 * D * n);
    uint32_t* dsp = buf<uint32_t>(ctx, "hx_sp", 32 * D * n);
    uint8_t* iok = buf<uint8_t>(ctx, "hx_ok", items);
    decrypt_device(ctx, D, n, dsk, de1, dct, ds, dsp, iok, nullptr);
    d2h(ctx, s, ds, 32 * D * n);
    d2h(ctx, s_prime, dsp, 32 * D * n);
    if (ok) d2h(ctx, ok, iok, items);
    sync(ctx);
    return DKG_OK;
  });
}

// Full-mode ceremony: round 1 with the shares hybrid-encrypted to the sorted member keys, the
// receivers decrypting them in round 2 (timed inside ms_round1 / ms_round2), then rounds 2-5 on
// the decrypted shares exactly as in plaintext mode.
int dkg_ceremony_run_full_device(dkg_ctx* ctx, size_t n, size_t t, const void* d_a, const void* d_b, const void* d_r,
                                 const uint8_t* sk, const uint8_t* pk, dkg_ceremony_out* out) {
  return guarded(ctx, [&] {
    const int rc = ceremony_args(ctx, n, t, {out, sk, pk, d_r});
    if (rc) return rc;
    const size_t N = t + 1, items = 2 * n * n;
    uint32_t* dsk = upload_scalars(ctx, "fm_sk", sk, n);
    uint32_t* dpk = buf<uint32_t>(ctx, "fm_pk", 32 * n);
    h2d(ctx, dpk, pk, 32 * n);
    HCK(hipEventRecord(ctx->ev[0], ctx->stream));
    const Commitments cm = commitment_rows(ctx, n, N);
    uint32_t* ds = buf<uint32_t>(ctx, "cer_s", 32 * n * n);
    uint32_t* dsp = buf<uint32_t>(ctx, "cer_sp", 32 * n * n);
    // With chunk streams (not the serialised roofline pass) the share evaluation, the encryption and
    // the receivers' decryption run on the low-priority side stream beside the check pipeline:
    // nothing before the checks reads a share, so the pipeline's binomial, stepping and
    // recombination start on the commitments alone, and the checks (and round 3) wait for the
    // decrypted shares (wait_shares); the decode mask of the ciphertexts joins the dealer mask there.
    const bool side = ctx->nsub > 1 && ctx->verify_mode == 0;
    hipStream_t hy = side ? ctx->side : ctx->stream;
    round1_device(ctx, n, n, t, (const uint32_t*)d_a, (const uint32_t*)d_b, cm.E, cm.A, ds, dsp, false, side);
    uint32_t* e1 = buf<uint32_t>(ctx, "fm_e1", 32 * items);
    uint32_t* ct = buf<uint32_t>(ctx, "fm_ct", 32 * items);
    encrypt_device(ctx, n, n, dpk, ds, dsp, (const uint32_t*)d_r, e1, ct, hy, pk);  // committee.rs:169-172
    HCK(hipEventRecord(ctx->ev[1], ctx->stream));
    uint32_t* rs = buf<uint32_t>(ctx, "fm_s", 32 * n * n);
    uint32_t* rsp = buf<uint32_t>(ctx, "fm_sp", 32 * n * n);
    uint8_t* iok = buf<uint8_t>(ctx, "fm_iok", items);
    uint8_t* eok = buf<uint8_t>(ctx, "fm_eok", n);
    decrypt_device(ctx, n, n, dsk, e1, ct, rs, rsp, iok, eok, hy);  // committee.rs:282-286
    if (side) {
      HCK(hipEventRecord(ctx->shares_done, ctx->side));
      ctx->shares_pending = true;
    }
    ExtScope ext(ctx, n, N);
    RoundMasks m;
    m.e_ok = eok;
    receivers_rounds(ctx, n, t, cm.E, cm.A, rs, rsp, out, false, m);
    phase_collect(ctx, "full", FULL_PHASES, std::size(FULL_PHASES));
    ceremony_times(ctx, out, true);
    return DKG_OK;
  });
}

int dkg_ceremony_verify_full(dkg_ctx* ctx, size_t n, size_t t, const uint8_t* E, const uint8_t* A, const uint8_t* e1,
                             const uint8_t* ct, const uint8_t* sk, dkg_ceremony_out* out) {
  return guarded(ctx, [&] {
    const int rc = ceremony_args(ctx, n, t, {out, E, A, e1, ct, sk});
    if (rc) return rc;
    CeremonyInput in;
    in.E = E, in.A = A, in.e1 = e1, in.ct = ct, in.sk = sk;
    return verify_ceremony(ctx, n, t, in, out);
  });
}

int dkg_ctx_set_complaint_eval(dkg_ctx* ctx, int mode) {
  if (!ctx || mode < 0 || mode == 3 || mode > 4) return DKG_E_ARG;  // 3: dkg_ctx_last_complaint_eval's "calling pass"
  ctx->complaint_eval = mode;
  return DKG_OK;
}

// ProofOfMisbehaviour::generate for C complaints from host arrays (inside a guarded call; syncs)
static int complaints_prove_run(dkg_ctx* ctx, size_t C, const uint8_t* sk, const uint8_t* enc, const uint8_t* w,
                                uint8_t* proofs) {
  {
    hipStream_t st = ctx->stream;
    uint32_t* dsk = buf<uint32_t>(ctx, "cp_sk", 32 * C);
    uint32_t* denc = buf<uint32_t>(ctx, "cp_enc", 128 * C);
    uint32_t* dw = buf<uint32_t>(ctx, "cp_w", 64 * C);
    h2d(ctx, dsk, sk, 32 * C);
    h2d(ctx, denc, enc, 128 * C);
    h2d(ctx, dw, w, 64 * C);
    uint32_t* Pc = buf<uint32_t>(ctx, "cp_Pc", 32 * 2 * C);
    uint32_t* ls = buf<uint32_t>(ctx, "cp_ls", 32 * 4 * C);
    uint32_t* lb = buf<uint32_t>(ctx, "cp_lb", 4 * 4 * C);
    uint32_t* gs = buf<uint32_t>(ctx, "cp_gs", 32 * 3 * C);
    dkgk::cp_prep(C, dsk, denc, dw, Pc, ls, lb, gs, st);
    uint32_t* Pext = buf<uint32_t>(ctx, "cp_Pext", PTB * 2 * C);
    uint8_t* pok = buf<uint8_t>(ctx, "cp_pok", 2 * C);
    dkgk::decode_points(Pc, 2 * C, Pext, 2 * C, pok, st);
    // K = sk e1 (recover_symmetric_key, broadcast.rs:197-202) and the announcements e1 w; pk = g sk, g w
    uint32_t* T = buf<uint32_t>(ctx, "cv_T", 4 * dkgk::cmp_ladder_table_words(4 * C));
    uint32_t* Lx = buf<uint32_t>(ctx, "cp_L", PTB * 4 * C);
    uint32_t* Gx = buf<uint32_t>(ctx, "cp_G", PTB * 3 * C);
    dkgk::cmp_ladder(4 * C, false, lb, nullptr, ls, nullptr, Pext, 2 * C, T, Lx, st);
    dkgk::fixed_base(3 * C, gs, ctx->tab_gw, Gx, st);
    uint32_t* lc = buf<uint32_t>(ctx, "cp_lc", 32 * 4 * C);
    uint32_t* gc = buf<uint32_t>(ctx, "cp_gc", 32 * 3 * C);
    dkgk::encode_points(Lx, 4 * C, 4 * C, lc, st);
    dkgk::encode_points(Gx, 3 * C, 3 * C, gc, st);
    uint32_t* dprf = buf<uint32_t>(ctx, "cp_proofs", 192 * C);
    dkgk::cp_finish(C, denc, lc, gc, gs, dprf, st);
    check_launch(ctx);
    std::vector<uint8_t> ok(2 * C);
    d2h(ctx, ok.data(), pok, 2 * C);
    d2h(ctx, proofs, dprf, 192 * C);
    sync(ctx);
    for (auto v : ok)
      if (!v) {
        ctx->err = "complaints_prove: a ciphertext point does not decode";
        return DKG_E_DECODE;
      }
    return DKG_OK;
  }
}

int dkg_complaints_prove(dkg_ctx* ctx, size_t C, const uint8_t* sk, const uint8_t* enc, const uint8_t* w,
                         uint8_t* proofs) {
  return guarded(ctx, [&] {
    if (!sk || !enc || !w || !proofs) return DKG_E_ARG;
    if (!C) return DKG_OK;
    return complaints_prove_run(ctx, C, sk, enc, w, proofs);
  });
}

// ---- one party's share checks (receivers.hip): P_i(x) for a few receiver indices, chunked Horner
int dkg_ctx_set_receiver_chunk(dkg_ctx* ctx, int chunk) {
  if (!ctx || chunk < 0) return DKG_E_ARG;
  ctx->receiver_chunk = chunk;
  return DKG_OK;
}

int dkg_ctx_last_receiver_chunk(const dkg_ctx* ctx) { return ctx ? ctx->last_receiver_chunk : 0; }

namespace {

constexpr size_t RECV_SLAB_BYTES = (size_t)256 << 20;      // chunk partials held at a time

// Field multiplication of the evaluation's launches when dkg_ctx_set_field_mode leaves the choice
// open: 1 column sums (dkgk_ilp), 0 product scanning (A/B in profiles/receivers_time.json).
#ifndef DKG_RECV_ILP
#define DKG_RECV_ILP 1
#endif

// The phases of a one-party, pairs or seats call (recv.*, pairs.*, seats.*), in the order a call passes them: the
// decryption (round 2; its closing mark opens a call that has none), the commitments decoded, the chunk walk done
// (the whole evaluation where no one launch sequence covers the call), folded, decided, the proofs (round 2).
// "recv" names the walk `chunks`, "seats" walk and folds together `eval`; `prove` is round2_tail's own collect.
enum { CP_DECRYPT, CP_DECODE, CP_WALK, CP_FOLD, CP_CHECK, CP_PROVE };
const PhaseRow RECV_PHASES[] = {{"decrypt", 1u << CP_DECRYPT}, {"decode", 1u << CP_DECODE}, {"chunks", 1u << CP_WALK},
                                {"fold", 1u << CP_FOLD},       {"check", 1u << CP_CHECK},   {"prove", 1u << CP_PROVE}};
const PhaseRow SEATS_PHASES[] = {{"decrypt", 1u << CP_DECRYPT}, {"decode", 1u << CP_DECODE},
                                 {"eval", 1u << CP_WALK | 1u << CP_FOLD}, {"fold", 1u << CP_FOLD},
                                 {"check", 1u << CP_CHECK},     {"prove", 1u << CP_PROVE}};
const PhaseRow PAIRS_PHASES[] = {{"decode", 1u << CP_DECODE}, {"eval", 1u << CP_WALK}};
const PhaseRow PROVE_PHASES[] = {{"prove", 1u << CP_PROVE}};

// Compressed rows Cc [..][N][32] on the device, decoded: the `rows` rows that dlist (device, may be null:
// the first `rows`) names, in that order.  Cext [rows * N] points at stride rows * N, pok per point, rowok
// per row; Cpm the position-major table [40][N][pad64(rows)] when asked for.
struct Decoded {
  uint32_t* Cext = nullptr;
  uint8_t *pok = nullptr, *rowok = nullptr;
  uint32_t* Cpm = nullptr;
};
void decode_stage(dkg_ctx* ctx, const uint32_t* Cc, const uint32_t* dlist, size_t rows, size_t N, bool pm,
                  Decoded& d) {
  hipStream_t st = ctx->stream;
  if (dlist) {
    uint32_t* gc = buf<uint32_t>(ctx, "dc_rows", 32 * rows * N);
    dkgk::gather_rows(rows, N, dlist, Cc, nullptr, gc, st);
    Cc = gc;
  }
  d.Cext = buf<uint32_t>(ctx, "Cext", PTB * rows * N);
  d.pok = buf<uint8_t>(ctx, "pok", rows * N);
  d.rowok = buf<uint8_t>(ctx, "dok", rows);
  dkgk::decode_points(Cc, rows * N, d.Cext, rows * N, d.pok, st);
  dkgk::dealer_ok(rows, N, d.pok, d.rowok, st);
  if (pm) {
    d.Cpm = buf<uint32_t>(ctx, "Cpm", PTB * N * pad64(rows));
    dkgk::to_position_major(rows, N, pad64(rows), d.Cext, d.Cpm, st);
  }
}

struct RecvEval {
  uint32_t* R = nullptr;    // [M * D][40] point-major, slot m's values at m * D + i
  uint8_t* dok = nullptr;   // [D] rows that decode
  uint32_t* xs = nullptr;   // [M] device: the 1-based indices (null: not uploaded)
  bool want_xs = true;      // in: the caller reads xs (recv_decide)
  // the plans of the M indices and their host staging (recv_plans): lives with the caller until it has synchronised
  std::vector<dkg_receiver_plan> plans;
  std::vector<uint32_t> hx, dig;
  bool any_stage = false;
};

const size_t RECV_DIG_STRIDE = fold_record(1, 16, 0);  // per index: a plan has 16 stages at most

// The plans of dkg_receiver_plan_for for the M indices js[m] + 1 (nplan = the n its cost rule sees), their 1-based
// indices and fold records: host only.
int recv_plans(dkg_ctx* ctx, size_t t, size_t M, const uint32_t* js, size_t nplan, RecvEval& ev) {
  const size_t N = t + 1;
  const size_t dig_stride = RECV_DIG_STRIDE;
  std::vector<dkg_receiver_plan>& plans = ev.plans;
  std::vector<uint32_t>&hx = ev.hx, &dig = ev.dig;
  plans.assign(M, dkg_receiver_plan());
  hx.assign(M, 0);
  dig.clear();
  int last = 0;
  bool any_stage = false;
  auto plan_of = [&](uint32_t x, int chunk, dkg_receiver_plan& out) {
    const std::array<size_t, 4> key = {std::max(nplan, (size_t)x), t, x, (size_t)chunk};
    auto it = ctx->recv_plans.find(key);
    if (it == ctx->recv_plans.end()) {
      dkg_receiver_plan p;
      const int rc = dkg_receiver_plan_for(key[0], t, x, chunk, &p);
      if (rc) return rc;
      if (ctx->recv_plans.size() >= 4096) ctx->recv_plans.clear();
      it = ctx->recv_plans.emplace(key, p).first;
    }
    out = it->second;
    return (int)DKG_OK;
  };
  // Several indices with the automatic choice: all take the largest of their automatic chunks (forced
  // plans of the same function), so that the slots have one shape and share every launch -- the fold's
  // work falls with the chunk, and such a call is bound by throughput, not by the chain.
  int chunk = ctx->receiver_chunk;
  if (M > 1 && chunk == 0) {
    for (size_t m = 0; m < M; m++) {
      dkg_receiver_plan p;
      const int rc = plan_of(js[m] + 1, 0, p);
      if (rc) return rc;
      chunk = std::max(chunk, (int)std::min<size_t>(p.chunk, N));
    }
  }
  for (size_t m = 0; m < M; m++) {
    hx[m] = js[m] + 1;
    const int rc = plan_of(hx[m], chunk, plans[m]);
    if (rc) return rc;
    if (plans[m].stages && dig.empty()) dig.assign(M * dig_stride, 0);
    if (plans[m].stages) fold_records(plans[m], &dig[m * dig_stride]);
    any_stage |= plans[m].stages != 0;
    last = std::max(last, (int)std::min<uint32_t>(plans[m].chunk, 0x7fffffffu));
  }
  ctx->last_receiver_chunk = last;
  ev.any_stage = any_stage;
  return DKG_OK;
}

// The evaluation half: every row of a prepared position-major table Cpm [40][N][pad64(D)] (padding columns valid
// points), rowok [D], at the M indices by ev's plans (recv_plans).  Marks, under `tag`, CP_DECODE (which closes the
// caller's preparation), CP_WALK and, where one slab of one plan covers the call so that one mark separates the
// chunk walk from the folds, CP_FOLD.
int recv_eval_table(dkg_ctx* ctx, const char* tag, size_t D, size_t t, size_t M, const uint32_t* Cpm, uint8_t* rowok,
                    RecvEval& ev) {
  const size_t N = t + 1, npad = pad64(D);
  const size_t dig_stride = RECV_DIG_STRIDE;
  const std::vector<dkg_receiver_plan>& plans = ev.plans;
  const std::vector<uint32_t>&hx = ev.hx, &dig = ev.dig;
  const bool any_stage = ev.any_stage;
  ev.dok = rowok;
  uint32_t* ddig = nullptr;
  if (any_stage || ev.want_xs) ev.xs = upload_words(ctx, "rv_xs", hx);  // the serial walk of one index reads neither
  if (any_stage) ddig = upload_words(ctx, "rv_dig", dig);
  ev.R = buf<uint32_t>(ctx, "rv_R", PTB * M * D);
  phase_mark_serial(ctx, tag, CP_DECODE);
  bool split = false;
  const bool ilp = ctx->fe_mode == 2 || (ctx->fe_mode == 0 && DKG_RECV_ILP);
  auto chunks = ilp ? dkgk_ilp::recv_chunks : dkgk::recv_chunks;
  auto fold = ilp ? dkgk_ilp::recv_fold : dkgk::recv_fold;
  size_t launches = 0;
  for (size_t m0 = 0; m0 < M;) {
    const dkg_receiver_plan& p = plans[m0];
    if (p.stages == 0) {  // the serial walk: k_horner, as dkg_verify_receiver runs it
      dkgk::horner(D, npad, N, Cpm, hx[m0], 1, ev.R + m0 * D * PT_WORDS_H, ctx->stream);
      m0++, launches++;
      continue;
    }
    const size_t L = p.chunk, G = (N + L - 1) / L;
    size_t run = 1;  // consecutive slots with the same shape share their launches
    while (m0 + run < M && plans[m0 + run].chunk == p.chunk && plans[m0 + run].stages == p.stages &&
           !memcmp(plans[m0 + run].arity, p.arity, sizeof p.arity))
      run++;
    const size_t Ms = std::min(run, std::max<size_t>(1, RECV_SLAB_BYTES / (PTB * G * npad)));
    const size_t G1 = (G + p.arity[0] - 1) / p.arity[0];
    uint32_t* Q[2] = {buf<uint32_t>(ctx, "rv_q0", PTB * Ms * G * npad), buf<uint32_t>(ctx, "rv_q1", PTB * Ms * G1 * npad)};
    for (size_t b = 0; b < run; b += Ms) {
      const size_t ms = std::min(Ms, run - b);
      chunks(D, npad, N, L, Cpm, ev.xs, m0 + b, ms, Q[0], ev.R, ctx->stream);
      if (launches == 0 && run == M && ms == run) {
        phase_mark_serial(ctx, tag, CP_WALK);
        split = true;
      }
      size_t Gin = G;
      for (uint32_t s = 0; s < p.stages; s++) {
        fold(D, npad, Gin, p.arity[s], Q[s & 1], ddig + fold_record(0, p.stages, s), dig_stride, m0 + b, ms,
             Q[(s + 1) & 1], ev.R, ctx->stream);
        Gin = (Gin + p.arity[s] - 1) / p.arity[s];
      }
      if (Gin != 1) {
        ctx->err = "receiver plan does not end in one value";
        return DKG_E_ARG;
      }
      launches++;
    }
    m0 += run;
  }
  check_launch(ctx);
  phase_mark_serial(ctx, tag, split ? CP_FOLD : CP_WALK);
  return DKG_OK;
}

// Decode C [D][N][32] and evaluate every row at the M indices js[m] + 1 by the plans of
// dkg_receiver_plan_for (nplan = the n its cost rule sees).  Marks recv.decode, .chunks and, where one slab of one
// plan covers the call so that one mark separates the chunk walk from the folds, .fold.
int recv_eval(dkg_ctx* ctx, size_t D, size_t t, size_t M, const uint32_t* js, size_t nplan, const uint8_t* C,
              RecvEval& ev) {
  const size_t N = t + 1;
  const int rc = recv_plans(ctx, t, M, js, nplan, ev);
  if (rc) return rc;
  phase_mark_serial(ctx, "recv", CP_DECRYPT);
  uint32_t* Cc = buf<uint32_t>(ctx, "vr_C", 32 * D * N);
  h2d(ctx, Cc, C, 32 * D * N);
  Decoded dc;
  decode_stage(ctx, Cc, nullptr, D, N, true, dc);
  return recv_eval_table(ctx, "recv", D, t, M, dc.Cpm, dc.rowok, ev);
}

// decisions [M][n] of the evaluated slots against the share columns (device, [M][n][8])
void recv_check(dkg_ctx* ctx, size_t n, int round, size_t M, size_t j0, const RecvEval& ev, const uint32_t* ds,
                const uint32_t* dsp, const uint8_t* qualified, uint8_t* dec) {
  if (M == 1) {  // one column: check's own mask and self index, as dkg_verify_receiver calls it
    dkgk::check(n, 1, 0, j0, n, round, ds, dsp, ev.R, ctx->tab_gw, ctx->tab_hw, ev.dok, dec, ctx->stream);
  } else {
    uint8_t* ones = buf<uint8_t>(ctx, "rv_one", M * n);
    HCK(hipMemsetAsync(ones, 1, M * n, ctx->stream));
    // pair p = m * n + i as "dealer" p of one receiver; recv_base = n keeps check's self test off
    dkgk::check(M * n, 1, 0, n, n, round, ds, dsp, ev.R, ctx->tab_gw, ctx->tab_hw, ones, dec, ctx->stream);
  }
  if (M > 1 || qualified) dkgk::recv_decide(M, n, round, ev.xs, ev.dok, qualified, dec, ctx->stream);
  check_launch(ctx);
  phase_mark_serial(ctx, "recv", CP_CHECK);
}

// The end of a round-2 call over S seats (dkg_party_round2: S = 1) once its decisions dec [S][n] are on the host:
// complaints[p] and r2_error[p] per seat (either may be null) and, with w, the proofs [S][n][192] of the rejected
// dealers -- all seats in one run, zero elsewhere, <tag>.prove its time.  sk [S][32]; e1, ct, w [S][n][64].
int round2_tail(dkg_ctx* ctx, const char* tag, size_t n, size_t t, size_t S, const uint8_t* dec, const uint8_t* sk,
                const uint8_t* e1, const uint8_t* ct, const uint8_t* w, int32_t* complaints, uint8_t* r2_error,
                uint8_t* proofs) {
  std::vector<size_t> rej;  // (seat, dealer) pairs p * n + i
  for (size_t p = 0; p < S; p++) {
    size_t cnt = 0;
    for (size_t i = 0; i < n; i++)
      if (dec[p * n + i] == DKG_REJECT) rej.push_back(p * n + i), cnt++;
    if (complaints) complaints[p] = (int32_t)cnt;
    if (r2_error) r2_error[p] = cnt > t ? 1 : 0;  // committee.rs:340-347
  }
  if (!w) return DKG_OK;
  memset(proofs, 0, 192 * S * n);
  if (rej.empty()) return DKG_OK;
  // ProofOfMisbehaviour::generate per rejected dealer (:309-322)
  const size_t Cn = rej.size();
  std::vector<uint8_t> ksk(32 * Cn), kenc(128 * Cn), kw(64 * Cn), kp(192 * Cn);
  for (size_t c = 0; c < Cn; c++) {
    const size_t e = rej[c];
    memcpy(&ksk[32 * c], sk + 32 * (e / n), 32);
    memcpy(&kenc[128 * c], e1 + 64 * e, 32);             // e1 of the randomness
    memcpy(&kenc[128 * c + 32], ct + 64 * e, 32);
    memcpy(&kenc[128 * c + 64], e1 + 64 * e + 32, 32);   // e1 of the share
    memcpy(&kenc[128 * c + 96], ct + 64 * e + 32, 32);
    memcpy(&kw[64 * c], w + 64 * e, 64);
  }
  phase_mark_serial(ctx, tag, -1);
  const int rp = complaints_prove_run(ctx, Cn, ksk.data(), kenc.data(), kw.data(), kp.data());
  if (rp) return rp;
  phase_mark_serial(ctx, tag, CP_PROVE);
  sync(ctx);
  phase_collect(ctx, tag, PROVE_PHASES, std::size(PROVE_PHASES));
  for (size_t c = 0; c < Cn; c++) memcpy(proofs + 192 * rej[c], &kp[192 * c], 192);
  return DKG_OK;
}

void recv_reset_last(dkg_ctx* ctx) {
  ctx->last_step_flags = nullptr;  // no stepping tables
  ctx->last_step_flag_words = 0;
  ctx->last_bflags = nullptr;
  ctx->last_bflag_words = 0;
}

}  // namespace

int dkg_commitment_eval(dkg_ctx* ctx, size_t D, size_t t, size_t M, const uint32_t* js, const uint8_t* C, uint8_t* P,
                        uint8_t* ok) {
  return guarded(ctx, [&] {
    if (!D || !M) return DKG_OK;
    if (!js || !C || !P) return DKG_E_ARG;
    for (size_t m = 0; m < M; m++)
      if (js[m] >= (1u << 24)) return DKG_E_ARG;
    recv_reset_last(ctx);
    RecvEval ev;
    const int rc = recv_eval(ctx, D, t, M, js, D, C, ev);
    if (rc) return rc;
    uint32_t* Pc = buf<uint32_t>(ctx, "rv_P", 32 * M * D);
    dkgk::recv_encode(M, D, ev.R, ev.dok, Pc, ctx->stream);
    check_launch(ctx);
    d2h(ctx, P, Pc, 32 * M * D);
    if (ok) d2h(ctx, ok, ev.dok, D);
    sync(ctx);
    phase_collect(ctx, "recv", RECV_PHASES, std::size(RECV_PHASES));
    return DKG_OK;
  });
}

// ---- public shares from the broadcast commitments (pubshares.hip)
int dkg_ctx_set_public_share_slab(dkg_ctx* ctx, size_t rows) {
  if (!ctx || rows > ((size_t)1 << 30)) return DKG_E_ARG;
  ctx->ps_slab = rows;
  return DKG_OK;
}

namespace {

// the phases of a public-shares call: the evaluator's ids (recv_eval_table marks them) and two of its own
enum { PS_SUM = 6, PS_DISCLOSED = 7 };
const PhaseRow PS_PHASES[] = {{"decode", 1u << CP_DECODE}, {"sum", 1u << PS_SUM},
                              {"eval", 1u << CP_WALK | 1u << CP_FOLD}, {"disclosed", 1u << PS_DISCLOSED}};

struct CommitSum {
  uint32_t* Sacc = nullptr;  // [40][N][bpad] position-major over the ceremonies, padding columns the identity
  uint8_t* ok = nullptr;     // [B] device: no used row of the ceremony is absent or undecodable
  size_t bpad = 0;
};

// S_c[k] = the sum over the used dealers i of A_{c,i}[k], for B ceremonies (A [B * n][N][32], host): the rows are
// uploaded and decoded in slabs (ctx->ps_slab, or as many as RECV_SLAB_BYTES of decoded points hold) and summed
// column by column into cs.Sacc (k_commit_colsum); a slab may cut through a ceremony.  use [B * n] (host, may be
// null: all used): commit_colsum's codes.  hrowok (host [B * n], may be null) receives "the row decodes" after the
// caller's sync.  Marks pubshares' decode and sum per slab.
void commit_sum_run(dkg_ctx* ctx, size_t B, size_t n, size_t N, const uint8_t* A, const uint8_t* use, uint8_t* hrowok,
                    CommitSum& cs) {
  hipStream_t st = ctx->stream;
  const size_t total = B * n;
  cs.bpad = pad64(B);
  cs.Sacc = buf<uint32_t>(ctx, "ps_S", PTB * N * cs.bpad);
  cs.ok = buf<uint8_t>(ctx, "ps_ok", B);
  dkgk::fill_identity(N * cs.bpad, cs.Sacc, st);
  HCK(hipMemsetAsync(cs.ok, 1, B, st));
  const uint8_t* duse = upload_mask(ctx, "ps_use", use, total);
  const size_t slab =
      std::min(total, ctx->ps_slab ? ctx->ps_slab : std::max<size_t>(1, RECV_SLAB_BYTES / (2 * PTB * N)));
  uint32_t* Cc = buf<uint32_t>(ctx, "ps_C", 32 * slab * N);
  phase_mark_serial(ctx, "pubshares", -1);
  for (size_t r0 = 0; r0 < total; r0 += slab) {
    const size_t rows = std::min(slab, total - r0);
    h2d(ctx, Cc, A + 32 * N * r0, 32 * N * rows);
    Decoded dc;
    decode_stage(ctx, Cc, nullptr, rows, N, true, dc);
    phase_mark_serial(ctx, "pubshares", CP_DECODE);
    dkgk::commit_colsum(n, N, r0, rows, pad64(rows), dc.Cpm, dc.rowok, duse, cs.bpad, cs.Sacc, cs.ok, st);
    if (hrowok) d2h(ctx, hrowok + r0, dc.rowok, rows);
    phase_mark_serial(ctx, "pubshares", PS_SUM);
  }
  check_launch(ctx);
}

// The encodings of cs.Sacc, queued: staging [N][bpad][32] (host) is read by commit_sum_store after the sync
void commit_sum_fetch(dkg_ctx* ctx, size_t N, const CommitSum& cs, std::vector<uint8_t>& staging) {
  const size_t count = N * cs.bpad;
  uint32_t* Sc = buf<uint32_t>(ctx, "ps_Sc", 32 * count);
  dkgk::encode_points(cs.Sacc, count, count, Sc, ctx->stream);
  check_launch(ctx);
  staging.resize(32 * count);
  d2h(ctx, staging.data(), Sc, 32 * count);
}
// S [B][N][32] from the staging; row c zero where hok[c] == 0
void commit_sum_store(size_t B, size_t N, size_t bpad, const std::vector<uint8_t>& staging, const uint8_t* hok,
                      uint8_t* S) {
  for (size_t c = 0; c < B; c++)
    for (size_t k = 0; k < N; k++) {
      if (hok[c]) memcpy(S + 32 * (c * N + k), &staging[32 * (k * bpad + c)], 32);
      else memset(S + 32 * (c * N + k), 0, 32);
    }
}

}  // namespace

int dkg_commitment_sum(dkg_ctx* ctx, size_t B, size_t n, size_t t, const uint8_t* A, const uint8_t* mask, uint8_t* S,
                       uint8_t* ok) {
  return guarded(ctx, [&] {
    if (!B) return DKG_OK;
    if (!n || !A || !S || B > 0xffffffffu / n) return DKG_E_ARG;
    recv_reset_last(ctx);
    const size_t N = t + 1;
    std::vector<uint8_t> use;
    if (mask) {
      use.resize(B * n);
      for (size_t e = 0; e < B * n; e++) use[e] = mask[e] ? 1 : 0;
    }
    CommitSum cs;
    commit_sum_run(ctx, B, n, N, A, mask ? use.data() : nullptr, nullptr, cs);
    std::vector<uint8_t> staging, hok(B);
    commit_sum_fetch(ctx, N, cs, staging);
    d2h(ctx, hok.data(), cs.ok, B);
    sync(ctx);
    phase_collect(ctx, "pubshares", PS_PHASES, std::size(PS_PHASES));
    commit_sum_store(B, N, cs.bpad, staging, hok.data(), S);
    if (ok) memcpy(ok, hok.data(), B);
    return DKG_OK;
  });
}

int dkg_public_shares(dkg_ctx* ctx, size_t B, size_t n, size_t t, const uint8_t* A, const uint8_t* qualified,
                      const uint8_t* reconstruct, const uint8_t* fetched3, size_t M, const uint32_t* js, size_t D5,
                      const uint32_t* d_ceremony, const uint32_t* d_sender, const uint32_t* d_dealer,
                      const uint8_t* d_share, uint8_t* V, int32_t* status, int32_t* which, uint8_t* S) {
  return guarded(ctx, [&] {
    if (!B || !M) return DKG_OK;
    if (!n || !A || !qualified || !js || !V || !status) return DKG_E_ARG;
    if (D5 && (!d_ceremony || !d_sender || !d_dealer || !d_share)) return DKG_E_ARG;
    // party indices are multipliers below 2^24 on the device; rows and list places are 32-bit
    if (n >= ((size_t)1 << 24) || B > 0xffffffffu / n || M >= 0xffffffffu || D5 >= 0xffffffffu) return DKG_E_ARG;
    for (size_t m = 0; m < M; m++)
      if (js[m] >= n) return DKG_E_ARG;
    for (size_t d = 0; d < D5; d++)
      if (d_ceremony[d] >= B || d_sender[d] < 1 || d_sender[d] > n || d_dealer[d] < 1 || d_dealer[d] > n)
        return DKG_E_ARG;
    const size_t N = t + 1, total = B * n;
    // the dealers the sum uses, and per ceremony how many are reconstructed
    std::vector<uint8_t> use(total);
    std::vector<uint32_t> nrec(B, 0);
    for (size_t c = 0; c < B; c++)
      for (size_t i = 0; i < n; i++) {
        const size_t e = c * n + i;
        const bool r = reconstruct && reconstruct[e];
        if (r && !qualified[e]) {
          ctx->err = "public_shares: only qualified members should be reconstructed (committee.rs:746-747 panics)";
          return DKG_E_ARG;
        }
        nrec[c] += r;
        use[e] = qualified[e] && !r ? (fetched3 && !fetched3[e] ? 2 : 1) : 0;
      }
    // the disclosed shares of the reconstructed dealers, summed per (ceremony, distinct index)
    std::vector<uint32_t> dj, place;
    dkgh::distinct_places(M, js, dj, place);
    const size_t Md = dj.size();
    constexpr uint32_t NONE = 0xffffffffu;
    std::vector<uint32_t> jslot(n, NONE);
    for (size_t k = 0; k < Md; k++) jslot[dj[k]] = (uint32_t)k;
    auto key = [&](size_t c, uint32_t sender0, uint32_t dealer0) { return ((uint64_t)c * n + sender0) * n + dealer0; };
    std::unordered_set<uint64_t> seen;
    seen.reserve(2 * D5);
    std::vector<dkgh::Zl> sums;
    std::vector<uint32_t> cnt;
    size_t kept = 0;
    for (size_t d = 0; d < D5; d++) {
      const size_t c = d_ceremony[d];
      const uint32_t q = d_sender[d] - 1, i = d_dealer[d] - 1;
      if (!seen.insert(key(c, q, i)).second) {
        ctx->err = "public_shares: a (ceremony, sender, dealer) disclosure is listed twice";
        return DKG_E_ARG;
      }
      if (!(reconstruct && reconstruct[c * n + i]) || jslot[q] == NONE) continue;
      if (sums.empty()) {
        sums.assign(B * Md, dkgh::zl_from_u64(0));
        cnt.assign(B * Md, 0);
      }
      const size_t at = c * Md + jslot[q];
      sums[at] = dkgh::zl_add(sums[at], dkgh::zl_from_bits(d_share + 32 * d));
      cnt[at]++;
      kept++;
    }
    recv_reset_last(ctx);
    hipStream_t st = ctx->stream;
    RecvEval ev;
    ev.want_xs = false;
    const int rp = recv_plans(ctx, t, M, js, B, ev);  // the cost rule sees the evaluator's rows: B ceremonies
    if (rp) return rp;
    // ---- S_c, then sum_k (j+1)^k S_c[k] with the ceremonies as the evaluator's rows
    std::vector<uint8_t> hrowok(total), hok(B), staging;
    CommitSum cs;
    commit_sum_run(ctx, B, n, N, A, use.data(), hrowok.data(), cs);
    const int re = recv_eval_table(ctx, "pubshares", B, t, M, cs.Sacc, cs.ok, ev);
    if (re) return re;
    // ---- g times the disclosed shares
    uint32_t* G = nullptr;
    std::vector<uint8_t> hsc;
    if (kept) {
      hsc.assign(32 * B * M, 0);
      for (size_t c = 0; c < B; c++)
        for (size_t m = 0; m < M; m++) dkgh::zl_to_bytes(&hsc[32 * (c * M + m)], sums[c * Md + place[m]]);
      uint32_t* dsc = buf<uint32_t>(ctx, "ps_sc", 32 * B * M);
      h2d(ctx, dsc, hsc.data(), 32 * B * M);
      G = buf<uint32_t>(ctx, "ps_G", PTB * B * M);
      dkgk::fixed_base(B * M, dsc, ctx->tab_gw, G, st);
      check_launch(ctx);
      phase_mark_serial(ctx, "pubshares", PS_DISCLOSED);
    }
    uint32_t* Vd = buf<uint32_t>(ctx, "ps_V", 32 * B * M);
    dkgk::pubshare_out(B, M, ev.R, G, Vd, st);
    check_launch(ctx);
    d2h(ctx, V, Vd, 32 * B * M);
    d2h(ctx, hok.data(), cs.ok, B);
    if (S) commit_sum_fetch(ctx, N, cs, staging);
    sync(ctx);
    phase_collect(ctx, "pubshares", PS_PHASES, std::size(PS_PHASES));
    if (S) commit_sum_store(B, N, cs.bpad, staging, hok.data(), S);
    // ---- dkg_public_share_status per (ceremony, index)
    for (size_t c = 0; c < B; c++) {
      int32_t absent = -1;  // the lowest used dealer without a usable row
      for (size_t i = 0; i < n && absent < 0; i++)
        if (use[c * n + i] == 2 || (use[c * n + i] == 1 && !hrowok[c * n + i])) absent = (int32_t)i;
      for (size_t m = 0; m < M; m++) {
        int32_t stt = DKG_PS_OK, w = -1;
        if (absent >= 0) {
          stt = DKG_PS_NO_COMMITMENT, w = absent;
        } else if (nrec[c] && (cnt.empty() || cnt[c * Md + place[m]] < nrec[c])) {
          stt = DKG_PS_NO_DISCLOSURE;
          for (size_t i = 0; i < n; i++)
            if (reconstruct[c * n + i] && !seen.count(key(c, js[m], (uint32_t)i))) {
              w = (int32_t)i;
              break;
            }
        }
        status[c * M + m] = stt;
        if (which) which[c * M + m] = w;
        if (stt != DKG_PS_OK) memset(V + 32 * (c * M + m), 0, 32);
      }
    }
    return DKG_OK;
  });
}

int dkg_commitment_eval_pairs(dkg_ctx* ctx, size_t D, size_t t, size_t count, const uint32_t* rows, const uint32_t* js,
                              const uint8_t* C, uint8_t* P, uint8_t* ok) {
  return guarded(ctx, [&] {
    if (!count) return DKG_OK;
    if (!D || !rows || !js || !C || !P) return DKG_E_ARG;
    for (size_t p = 0; p < count; p++)
      if (rows[p] >= D || js[p] >= (1u << 24)) return DKG_E_ARG;
    uint32_t L, G, S;
    if (dkg_pair_eval_shape(t, ctx->receiver_chunk, &L, &G, &S) != DKG_OK) return DKG_E_ARG;
    recv_reset_last(ctx);
    const size_t N = t + 1;
    hipStream_t st = ctx->stream;
    std::vector<uint32_t> drows, crow, hx(count);
    dkgh::distinct_places(count, rows, drows, crow);
    for (size_t p = 0; p < count; p++) crow[p] += 1, hx[p] = js[p] + 1;  // 1-based, as k_cmp_horner's lists
    const size_t Rn = drows.size();
    phase_mark_serial(ctx, "pairs", -1);
    // the distinct rows gathered and decoded, as the batch complaint stage does it
    uint32_t* Cc = buf<uint32_t>(ctx, "vr_C", 32 * D * N);
    h2d(ctx, Cc, C, 32 * D * N);
    uint32_t* dlist = upload_words(ctx, "pe_rows", drows);
    uint32_t* dcrow = upload_words(ctx, "pe_crow", crow);
    uint32_t* dxs = upload_words(ctx, "pe_xs", hx);
    Decoded dc;
    decode_stage(ctx, Cc, dlist, Rn, N, false, dc);
    uint8_t* iok = buf<uint8_t>(ctx, "pe_ok", count);
    dkgk::pair_ok(count, dcrow, dc.rowok, iok, st);
    phase_mark_serial(ctx, "pairs", CP_DECODE);
    uint32_t* R = buf<uint32_t>(ctx, "pe_R", PTB * count);
    PairStage ps;
    pair_eval_launch(ctx, t, count, nullptr, hx.data(), dxs, dcrow, dc.Cext, Rn * N, R, ps);
    phase_mark_serial(ctx, "pairs", CP_WALK);
    uint32_t* Pc = buf<uint32_t>(ctx, "pe_P", 32 * count);
    dkgk::recv_encode(1, count, R, iok, Pc, st);
    check_launch(ctx);
    d2h(ctx, P, Pc, 32 * count);
    if (ok) d2h(ctx, ok, iok, count);
    sync(ctx);  // the staging vectors live until here
    phase_collect(ctx, "pairs", PAIRS_PHASES, std::size(PAIRS_PHASES));
    return DKG_OK;
  });
}

int dkg_verify_receivers(dkg_ctx* ctx, size_t n, size_t t, int round, size_t M, const uint32_t* js, const uint8_t* C,
                         const uint8_t* s, const uint8_t* s_prime, const uint8_t* qualified, uint8_t* decision) {
  return guarded(ctx, [&] {
    if (round != 2 && round != 4) return DKG_E_ARG;
    if (!M) return DKG_OK;
    if (!n || !js || !C || !s || !decision) return DKG_E_ARG;
    for (size_t m = 0; m < M; m++)
      if (js[m] >= n) return DKG_E_ARG;
    if (round == 2) {
      int rc = need_env(ctx);
      if (rc) return rc;
      if (!s_prime) return DKG_E_ARG;
    }
    recv_reset_last(ctx);
    RecvEval ev;
    ev.want_xs = M > 1 || (round == 4 && qualified);
    const int rc = recv_eval(ctx, n, t, M, js, n, C, ev);
    if (rc) return rc;
    uint32_t* ds = upload_scalars(ctx, "vr_s", s, M * n);
    uint32_t* dsp = round == 2 ? upload_scalars(ctx, "vr_sp", s_prime, M * n) : nullptr;
    const uint8_t* dq = round == 4 ? upload_mask(ctx, "rv_q", qualified, n) : nullptr;
    uint8_t* dec = buf<uint8_t>(ctx, "vr_dec", M * n);
    recv_check(ctx, n, round, M, js[0], ev, ds, dsp, dq, dec);
    d2h(ctx, decision, dec, M * n);
    sync(ctx);
    phase_collect(ctx, "recv", RECV_PHASES, std::size(RECV_PHASES));
    return DKG_OK;
  });
}

int dkg_party_round2(dkg_ctx* ctx, size_t n, size_t t, size_t j, const uint8_t* E, const uint8_t* e1, const uint8_t* ct,
                     const uint8_t sk[32], const uint8_t* w, uint8_t* s_out, uint8_t* sp_out, uint8_t* dec,
                     int32_t* complaints, uint8_t* r2_error, uint8_t* proofs) {
  return guarded(ctx, [&] {
    const int rc0 = ceremony_args(ctx, n, t, {E, e1, ct, sk, dec});
    if (rc0) return rc0;
    if (j >= n || (w && !proofs)) return DKG_E_ARG;
    recv_reset_last(ctx);
    // committee.rs:282-286: the pairs addressed to j, decrypted with sk_j (one recipient)
    phase_mark_serial(ctx, "recv", -1);
    uint32_t* dsk = upload_scalars(ctx, "pr_sk", sk, 1);
    uint32_t* de1 = buf<uint32_t>(ctx, "pr_e1", 64 * n);
    uint32_t* dct = buf<uint32_t>(ctx, "pr_ct", 64 * n);
    h2d(ctx, de1, e1, 64 * n);
    h2d(ctx, dct, ct, 64 * n);
    uint32_t* ds = buf<uint32_t>(ctx, "pr_s", 32 * n);
    uint32_t* dsp = buf<uint32_t>(ctx, "pr_sp", 32 * n);
    uint8_t* iok = buf<uint8_t>(ctx, "pr_iok", 2 * n);
    uint8_t* eok = buf<uint8_t>(ctx, "pr_eok", n);
    decrypt_device(ctx, n, 1, dsk, de1, dct, ds, dsp, iok, eok);
    const uint32_t jj = (uint32_t)j;
    RecvEval ev;
    ev.want_xs = false;
    const int rc = recv_eval(ctx, n, t, 1, &jj, n, E, ev);  // :287-296
    if (rc) return rc;
    dkgk::and_mask(n, eok, ev.dok, ctx->stream);  // an e1 that does not decode is missing data (:331-335)
    uint8_t* ddec = buf<uint8_t>(ctx, "vr_dec", n);
    recv_check(ctx, n, 2, 1, j, ev, ds, dsp, nullptr, ddec);
    d2h(ctx, dec, ddec, n);
    if (s_out) d2h(ctx, s_out, ds, 32 * n);
    if (sp_out) d2h(ctx, sp_out, dsp, 32 * n);
    sync(ctx);
    phase_collect(ctx, "recv", RECV_PHASES, std::size(RECV_PHASES));
    return round2_tail(ctx, "recv", n, t, 1, dec, sk, e1, ct, w, complaints, r2_error, proofs);
  });
}

// ---- hosted seats: one operator's share checks across many ceremonies (receivers.hip k_seat_horner)
// Field multiplication of k_seat_horner when dkg_ctx_set_field_mode leaves the choice open: 1 column sums
// (dkgk_ilp), 0 product scanning (A/B in profiles/seats_time.json).
#ifndef DKG_SEAT_ILP
#define DKG_SEAT_ILP 1
#endif

namespace {

struct SeatEval {
  dkgh::SeatPlan plan;         // host staging of the descriptors: lives until the caller has synchronised
  std::vector<uint32_t> rows;  // dealer rows of the distinct ceremonies
  uint32_t* R = nullptr;       // [S * n][40] point-major
  uint8_t* sok = nullptr;      // [S][n] dealer i's data decodes for seat p
  uint32_t* sx = nullptr;      // [S] device: the seats' 1-based indices
  uint32_t* scer = nullptr;    // [S] device: the seats' ceremonies
  std::vector<uint32_t> xslot, dig;  // chunked route: per-wave slot and the fold_records per distinct x
};

constexpr uint64_t SEAT_SCRATCH_MAX = (uint64_t)1 << 30;  // Q and its ping-pong partner

// Decode the distinct ceremonies the seats name (C [B * n][N][32]) and evaluate dealer i of seat p's
// ceremony at js[p] + 1 by dkg_seat_pack's waves.  extra (device [S][n], may be null) is ANDed into sok.
// The route is ctx->seat_eval's: k_seat_horner, or k_seat_chunks and k_seat_fold in dkg_seat_eval_shape's
// shape.  Marks seats.decode and the evaluation: the chunk walk and, when folded, the folds.
int seats_eval(dkg_ctx* ctx, size_t B, size_t n, size_t t, size_t S, const uint32_t* cer, const uint32_t* js,
               const uint8_t* C, const uint8_t* extra, SeatEval& ev) {
  if (B > 0xffffffffu / n) return DKG_E_ARG;  // dealer rows are 32-bit
  const int rc = dkgh::seat_plan(B, n, S, cer, js, ev.plan);
  if (rc) return rc;
  const dkgh::SeatPlan& pl = ev.plan;
  const size_t N = t + 1, Bd = pl.cers.size(), D = Bd * n, cols = pad64(D);
  // the route, before anything is uploaded: a forced shape may be refused
  uint32_t L = (uint32_t)std::min<size_t>(N, 0x7fffffffu), G = 1, stages = 0;
  uint64_t scratch = 0;
  if (ctx->seat_eval != 1 && pl.waves) {
    const uint32_t x_max = *std::max_element(pl.seat_x.begin(), pl.seat_x.end());
    const int rs = dkg_seat_eval_shape(n, t, pl.waves, x_max, ctx->seat_eval_chunk, &L, &G, &stages, &scratch);
    if (rs) {
      ctx->err = "seats: dkg_seat_eval_shape refuses chunk " + std::to_string(ctx->seat_eval_chunk);
      return rs;
    }
    if (scratch > SEAT_SCRATCH_MAX) {
      ctx->err = "seats: the forced chunk " + std::to_string(L) + " needs " + std::to_string(scratch) +
                 " bytes of scratch, more than " + std::to_string(SEAT_SCRATCH_MAX);
      return DKG_E_ARG;
    }
  }
  if (G > 1) {  // one digit record per (distinct x, stage); the waves name their x's records
    std::vector<uint32_t> wx(pl.waves), xs;
    for (size_t v = 0; v < pl.waves; v++) wx[v] = pl.wave_desc[2 * v];
    dkgh::distinct_places(pl.waves, wx.data(), xs, ev.xslot);
    ev.dig.assign(fold_record(xs.size(), stages, 0), 0);
    for (size_t k = 0; k < xs.size(); k++) {
      dkg_receiver_plan p;
      if (dkg_receiver_plan_for(n, t, xs[k], (int)L, &p) != DKG_OK || p.stages != stages) {
        ctx->err = "seats: no fold plan for index " + std::to_string(xs[k]);
        return DKG_E_ARG;
      }
      fold_records(p, &ev.dig[fold_record(k, stages, 0)]);
    }
  }
  ctx->last_seat_eval = G > 1 ? 2 : 1;
  ctx->last_seat_eval_chunk = (int)L;
  ev.rows.resize(D);
  for (size_t c = 0; c < Bd; c++)
    for (size_t i = 0; i < n; i++) ev.rows[c * n + i] = (uint32_t)(pl.cers[c] * n + i);
  hipStream_t st = ctx->stream;
  phase_mark_serial(ctx, "seats", CP_DECRYPT);
  uint32_t* Cc = buf<uint32_t>(ctx, "vr_C", 32 * B * n * N);
  h2d(ctx, Cc, C, 32 * B * n * N);
  uint32_t* drows = upload_words(ctx, "st_rows", ev.rows);
  uint32_t* dscol = upload_words(ctx, "st_scol", pl.seat_col);
  uint32_t* dwdesc = upload_words(ctx, "st_wdesc", pl.wave_desc);
  uint32_t* dwseat = upload_words(ctx, "st_wseat", pl.wave_seat);
  ev.sx = upload_words(ctx, "st_sx", pl.seat_x);
  ev.scer = buf<uint32_t>(ctx, "st_scer", 4 * S);
  h2d(ctx, ev.scer, cer, 4 * S);
  // only the ceremonies named are gathered and decoded, as the pair evaluation does with its rows
  Decoded dc;
  decode_stage(ctx, Cc, drows, D, N, true, dc);
  ev.sok = buf<uint8_t>(ctx, "st_sok", S * n);
  ev.R = buf<uint32_t>(ctx, "rv_R", PTB * S * n);
  dkgk::seat_ok(S, n, dscol, dc.rowok, extra, ev.sok, st);
  phase_mark_serial(ctx, "seats", CP_DECODE);
  const bool ilp = ctx->fe_mode == 2 || (ctx->fe_mode == 0 && DKG_SEAT_ILP);
  if (G == 1) {
    (ilp ? dkgk_ilp::seat_horner : dkgk::seat_horner)(pl.waves, n, N, cols, pl.width, dwdesc, dwseat, dscol, dc.Cpm,
                                                      ev.R, st);
  } else {
    uint32_t* dxslot = upload_words(ctx, "st_xslot", ev.xslot);
    uint32_t* ddig = upload_words(ctx, "st_dig", ev.dig);
    uint32_t* q0 = buf<uint32_t>(ctx, "st_q", scratch);  // 2 x [40][G][64 waves] words
    uint32_t* Q[2] = {q0, q0 + scratch / 8};
    (ilp ? dkgk_ilp::seat_chunks : dkgk::seat_chunks)(pl.waves, n, N, cols, pl.width, L, dwdesc, dwseat, dscol, dc.Cpm,
                                                      Q[0], st);
    phase_mark_serial(ctx, "seats", CP_WALK);
    size_t Gin = G;
    for (uint32_t s = 0; s < stages; s++) {
      (ilp ? dkgk_ilp::seat_fold : dkgk::seat_fold)(pl.waves, n, pl.width, Gin, dwdesc, dwseat, dxslot,
                                                    ddig + fold_record(0, stages, s), fold_record(1, stages, 0),
                                                    Q[s & 1], Q[(s + 1) & 1], ev.R, st);
      Gin = (Gin + 1) / 2;
    }
    if (Gin != 1) {
      ctx->err = "seats: the fold does not end in one value";
      return DKG_E_ARG;
    }
  }
  check_launch(ctx);
  phase_mark_serial(ctx, "seats", G == 1 ? CP_WALK : CP_FOLD);
  return DKG_OK;
}

// decisions [S][n] of the evaluated seats against their share columns (device, [S][n][8]); marks seats.check
void seats_check(dkg_ctx* ctx, size_t n, int round, size_t S, const SeatEval& ev, const uint32_t* ds,
                 const uint32_t* dsp, const uint8_t* qualified, uint8_t* dec) {
  // pair p * n + i as "dealer" of one receiver, as recv_check; recv_base = n keeps check's self test off
  dkgk::check(S * n, 1, 0, n, n, round, ds, dsp, ev.R, ctx->tab_gw, ctx->tab_hw, ev.sok, dec, ctx->stream);
  dkgk::seat_decide(S, n, round, ev.sx, ev.scer, ev.sok, qualified, dec, ctx->stream);
  check_launch(ctx);
  phase_mark_serial(ctx, "seats", CP_CHECK);
}

}  // namespace

int dkg_commitment_eval_seats(dkg_ctx* ctx, size_t B, size_t n, size_t t, size_t S, const uint32_t* cer,
                              const uint32_t* js, const uint8_t* C, uint8_t* P, uint8_t* ok) {
  return guarded(ctx, [&] {
    if (!S) return DKG_OK;
    if (!B || !n || !cer || !js || !C || !P) return DKG_E_ARG;
    recv_reset_last(ctx);
    SeatEval ev;
    const int rc = seats_eval(ctx, B, n, t, S, cer, js, C, nullptr, ev);
    if (rc) return rc;
    uint32_t* Pc = buf<uint32_t>(ctx, "rv_P", 32 * S * n);
    dkgk::recv_encode(1, S * n, ev.R, ev.sok, Pc, ctx->stream);  // one flag per (seat, dealer)
    check_launch(ctx);
    d2h(ctx, P, Pc, 32 * S * n);
    if (ok) d2h(ctx, ok, ev.sok, S * n);
    sync(ctx);
    phase_collect(ctx, "seats", SEATS_PHASES, std::size(SEATS_PHASES));
    return DKG_OK;
  });
}

int dkg_verify_seats(dkg_ctx* ctx, size_t B, size_t n, size_t t, int round, size_t S, const uint32_t* cer,
                     const uint32_t* js, const uint8_t* C, const uint8_t* s, const uint8_t* s_prime,
                     const uint8_t* qualified, uint8_t* decision) {
  return guarded(ctx, [&] {
    if (round != 2 && round != 4) return DKG_E_ARG;
    if (!S) return DKG_OK;
    if (!B || !n || !cer || !js || !C || !s || !decision) return DKG_E_ARG;
    if (round == 2) {
      int rc = need_env(ctx);
      if (rc) return rc;
      if (!s_prime) return DKG_E_ARG;
    }
    recv_reset_last(ctx);
    SeatEval ev;
    const int rc = seats_eval(ctx, B, n, t, S, cer, js, C, nullptr, ev);
    if (rc) return rc;
    uint32_t* ds = upload_scalars(ctx, "vr_s", s, S * n);
    uint32_t* dsp = round == 2 ? upload_scalars(ctx, "vr_sp", s_prime, S * n) : nullptr;
    const uint8_t* dq = round == 4 ? upload_mask(ctx, "rv_q", qualified, B * n) : nullptr;
    uint8_t* dec = buf<uint8_t>(ctx, "vr_dec", S * n);
    seats_check(ctx, n, round, S, ev, ds, dsp, dq, dec);
    d2h(ctx, decision, dec, S * n);
    sync(ctx);
    phase_collect(ctx, "seats", SEATS_PHASES, std::size(SEATS_PHASES));
    return DKG_OK;
  });
}

int dkg_party_round2_seats(dkg_ctx* ctx, size_t B, size_t n, size_t t, size_t S, const uint32_t* cer,
                           const uint32_t* js, const uint8_t* E, const uint8_t* e1, const uint8_t* ct,
                           const uint8_t* sk, const uint8_t* w, uint8_t* s_out, uint8_t* sp_out, uint8_t* dec,
                           int32_t* complaints, uint8_t* r2_error, uint8_t* proofs) {
  return guarded(ctx, [&] {
    if (!S) return DKG_OK;
    const int rc0 = ceremony_args(ctx, n, t, {E, e1, ct, sk, dec, cer, js});
    if (rc0) return rc0;
    if (!B || (w && !proofs)) return DKG_E_ARG;
    for (size_t p = 0; p < S; p++)
      if (cer[p] >= B || js[p] >= n) return DKG_E_ARG;  // before any launch
    recv_reset_last(ctx);
    hipStream_t st = ctx->stream;
    // committee.rs:282-286 for every seat: the n pairs addressed to seat p, decrypted with sk_p -- one wave
    // per (seat key, w, 64 dealers), the scalar wave-uniform (k_bdec_mul_w4's chain, seat-addressed)
    phase_mark_serial(ctx, "seats", -1);
    const size_t items = 2 * S * n;
    uint32_t* dsk = upload_scalars(ctx, "pr_sk", sk, S);
    uint32_t* de1 = buf<uint32_t>(ctx, "pr_e1", 32 * items);
    uint32_t* dct = buf<uint32_t>(ctx, "pr_ct", 32 * items);
    h2d(ctx, de1, e1, 32 * items);
    h2d(ctx, dct, ct, 32 * items);
    uint32_t* ds = buf<uint32_t>(ctx, "pr_s", 32 * S * n);
    uint32_t* dsp = buf<uint32_t>(ctx, "pr_sp", 32 * S * n);
    uint8_t* iok = buf<uint8_t>(ctx, "pr_iok", items);
    uint8_t* eok = buf<uint8_t>(ctx, "pr_eok", S * n);
    uint32_t* R = buf<uint32_t>(ctx, "hy.R", PTB * items);
    uint32_t* K = buf<uint32_t>(ctx, "hy.K", PTB * items);
    uint32_t* Kc = buf<uint32_t>(ctx, "hy.Kc", 32 * items);
    uint32_t* T = buf<uint32_t>(ctx, "bf.dec_tab", 4 * dkgk::bdec_mul_table_words(S, n));
    dkgk::decode_points(de1, items, R, items, iok, st);
    dkgk::seat_dec_mul(S, n, dsk, R, K, items, T, st);
    dkgk::encode_points(K, items, items, Kc, st);
    dkgk::sym_xor(S, n, Kc, true, dct, ds, dsp, st);
    dkgk::dealer_ok(S * n, 2, iok, eok, st);  // an e1 that does not decode is missing data (:331-335)
    check_launch(ctx);
    SeatEval ev;
    const int rc = seats_eval(ctx, B, n, t, S, cer, js, E, eok, ev);  // :287-296
    if (rc) return rc;
    uint8_t* ddec = buf<uint8_t>(ctx, "vr_dec", S * n);
    seats_check(ctx, n, 2, S, ev, ds, dsp, nullptr, ddec);
    d2h(ctx, dec, ddec, S * n);
    if (s_out) d2h(ctx, s_out, ds, 32 * S * n);
    if (sp_out) d2h(ctx, sp_out, dsp, 32 * S * n);
    sync(ctx);
    phase_collect(ctx, "seats", SEATS_PHASES, std::size(SEATS_PHASES));
    return round2_tail(ctx, "seats", n, t, S, dec, sk, e1, ct, w, complaints, r2_error, proofs);
  });
}

// ---- hosted seats deal round 1 (seat_deal.hip)
// K = pk r of a dealing seat when dkg_ctx_set_seat_deal leaves the choice open: 2 the joint chain, 1 the
// radix-16 combs per key slot (profiles/seat_deal_time.json).
#ifndef DKG_SEAT_DEAL_AUTO
#define DKG_SEAT_DEAL_AUTO 2
#endif

namespace {

enum { SD_COMMIT, SD_E1, SD_MUL, SD_ENCODE, SD_SYM, SD_PHASES };
// seats.commit and .deal_*: the call's device times, the hybrid kernels' summed over all chunks of seats
const PhaseRow SD_ROWS[SD_PHASES] = {{"commit", 1u << SD_COMMIT},
                                     {"deal_e1", 1u << SD_E1},
                                     {"deal_mul", 1u << SD_MUL},
                                     {"deal_encode", 1u << SD_ENCODE},
                                     {"deal_sym", 1u << SD_SYM}};

// Seats per chunk of the hybrid stage: the extended-form R and K, the K encodings and, on the comb route,
// the per-slot key copies, their gather index and their radix-16 combs within BFULL_SCRATCH_BYTES;
// dkg_ctx_set_batch_full_chunk forces a count (of seats, here).
size_t seat_deal_chunk(const dkg_ctx* ctx, size_t S, size_t n, int mode) {
  size_t per = 2 * n * (2 * PTB + 32);
  if (mode == 1) per += n * (PTB + 4 + 4 * dkgk::benc_tab_words());
  const size_t c = ctx->bfull_chunk ? ctx->bfull_chunk : std::max<size_t>(1, BFULL_SCRATCH_BYTES / per);
  return std::min(c, S);
}

}  // namespace

int dkg_party_round1_seats(dkg_ctx* ctx, size_t B, size_t n, size_t t, size_t S, const uint32_t* cer,
                           const uint32_t* js, const uint8_t* a, const uint8_t* b, const uint8_t* r,
                           const uint8_t* pk, uint8_t* E, uint8_t* A, uint8_t* e1, uint8_t* ct, uint8_t* s_out,
                           uint8_t* sp_out, uint8_t* own) {
  return guarded(ctx, [&] {
    if (!S) return DKG_OK;
    const int rc0 = ceremony_args(ctx, n, t, {cer, js, a, b, r, pk, E, A, e1, ct});
    if (rc0) return rc0;
    if (!B || B > 0xffffffffu / n || S > 0xffffffffu / (2 * n)) return DKG_E_ARG;  // keys and items are 32-bit
    for (size_t p = 0; p < S; p++)
      if (cer[p] >= B || js[p] >= n) return DKG_E_ARG;  // before any launch
    const int mode = ctx->seat_deal ? ctx->seat_deal : DKG_SEAT_DEAL_AUTO;
    ctx->last_seat_deal = mode;
    hipStream_t st = ctx->stream;
    const size_t N = t + 1;
    // the distinct ceremonies named, in order of first mention: only their keys are uploaded and decoded
    std::vector<uint32_t> cers, kbase(S);
    {
      std::map<uint32_t, uint32_t> slot_of;
      for (size_t p = 0; p < S; p++) {
        auto it = slot_of.find(cer[p]);
        if (it == slot_of.end()) {
          it = slot_of.emplace(cer[p], (uint32_t)cers.size()).first;
          cers.push_back(cer[p]);
        }
        kbase[p] = it->second * (uint32_t)n;
      }
    }
    const size_t Ck = cers.size() * n;
    std::vector<uint8_t> pkh(32 * Ck);
    for (size_t c = 0; c < cers.size(); c++) memcpy(&pkh[32 * c * n], pk + 32 * (size_t)cers[c] * n, 32 * n);
    uint32_t* dpk = buf<uint32_t>(ctx, "sd_pk", 32 * Ck);
    uint32_t* pk_ext = buf<uint32_t>(ctx, "sd_pk_ext", PTB * Ck);
    uint8_t* pk_ok = buf<uint8_t>(ctx, "sd_pk_ok", Ck);
    uint32_t* dkbase = buf<uint32_t>(ctx, "sd_kbase", 4 * S);
    h2d(ctx, dpk, pkh.data(), 32 * Ck);
    h2d(ctx, dkbase, kbase.data(), 4 * S);
    uint32_t* da = upload_scalars(ctx, "sd_a", a, S * N);
    uint32_t* db = upload_scalars(ctx, "sd_b", b, S * N);
    uint32_t* dr = upload_scalars(ctx, "sd_r", r, 2 * S * n);
    uint32_t* Ec = buf<uint32_t>(ctx, "sd_E", 32 * S * N);
    uint32_t* Ac = buf<uint32_t>(ctx, "sd_A", 32 * S * N);
    uint32_t* ds = buf<uint32_t>(ctx, "sd_s", 32 * S * n);
    uint32_t* dsp = buf<uint32_t>(ctx, "sd_sp", 32 * S * n);
    uint32_t* de1 = buf<uint32_t>(ctx, "sd_e1", 64 * S * n);
    uint32_t* dct = buf<uint32_t>(ctx, "sd_ct", 64 * S * n);
    dkgk::decode_points(dpk, Ck, pk_ext, Ck, pk_ok, st);
    auto mark = [&](int phase) { phase_mark_serial(ctx, "seats", phase); };
    mark(-1);
    round1_device(ctx, S, n, t, da, db, Ec, Ac, ds, dsp);  // committee.rs:141-167 with D = S dealers
    mark(SD_COMMIT);
    // :164-178 per seat: items (p, q, w) at (p * n + q) * 2 + w, in chunks of seats
    const size_t chunk = seat_deal_chunk(ctx, S, n, mode);
    const size_t mslots = chunk * n, mi = 2 * mslots;
    uint32_t* R = buf<uint32_t>(ctx, "bf.R", PTB * mi);
    uint32_t* K = buf<uint32_t>(ctx, "bf.K", PTB * mi);
    uint32_t* Kc = buf<uint32_t>(ctx, "bf.Kc", 32 * mi);
    uint32_t *idx = nullptr, *pks = nullptr, *tab = nullptr;
    if (mode == 1) {
      idx = buf<uint32_t>(ctx, "sd_idx", 4 * mslots);
      pks = buf<uint32_t>(ctx, "bf.pk_ext", PTB * mslots);
      tab = buf<uint32_t>(ctx, "bf.tab", 4 * dkgk::benc_tab_words() * mslots);
    }
    for (size_t p0 = 0; p0 < S; p0 += chunk) {
      const size_t Sc = std::min(chunk, S - p0), slots = Sc * n, items = 2 * slots;
      const size_t q0 = p0 * n, i0 = 2 * q0;  // first (seat, recipient) slot / item
      dkgk::fixed_base(items, dr + 8 * i0, ctx->tab_gw, R, st);  // e1 = G::generator() * r  (elgamal.rs:141)
      mark(SD_E1);
      if (mode == 1) {  // a comb per key slot: k_benc_tab, then k_benc_mul with one dealer row per key
        dkgk::seat_key_index(slots, n, dkbase + p0, idx, st);
        dkgk::seat_gather_points(slots, idx, pk_ext, Ck, pks, slots, st);
        dkgk::benc_tab(slots, pks, slots, tab, st);
        dkgk::benc_mul(slots, n, 1, dr + 8 * i0, tab, K, items, st);
      } else {          // key = pk * r  (elgamal.rs:138-140), both products of a slot on one lane
        dkgk::seat_enc_mul(slots, n, dkbase + p0, dr + 8 * i0, pk_ext, Ck, K, items, st);
      }
      mark(SD_MUL);
      dkgk::encode_points(R, items, items, de1 + 8 * i0, st);
      dkgk::encode_points(K, items, items, Kc, st);
      mark(SD_ENCODE);
      dkgk::sym_xor(Sc, n, Kc, false, dct + 8 * i0, ds + 8 * q0, dsp + 8 * q0, st);
      mark(SD_SYM);
    }
    check_launch(ctx);
    std::vector<uint8_t> okh(Ck), sh, sph;
    d2h(ctx, okh.data(), pk_ok, Ck);
    d2h(ctx, E, Ec, 32 * S * N);
    d2h(ctx, A, Ac, 32 * S * N);
    d2h(ctx, e1, de1, 64 * S * n);
    d2h(ctx, ct, dct, 64 * S * n);
    if (own && !s_out) sh.resize(32 * S * n), s_out = sh.data();
    if (own && !sp_out) sph.resize(32 * S * n), sp_out = sph.data();
    if (s_out) d2h(ctx, s_out, ds, 32 * S * n);
    if (sp_out) d2h(ctx, sp_out, dsp, 32 * S * n);
    sync(ctx);
    phase_collect(ctx, "seats", SD_ROWS, SD_PHASES);
    for (size_t k = 0; k < Ck; k++)
      if (!okh[k]) {
        ctx->err = "party_round1_seats: the key of recipient " + std::to_string(k % n) + " of ceremony " +
                   std::to_string(cers[k / n]) + " does not decode";
        return DKG_E_DECODE;
      }
    if (own)  // what init keeps as decrypted_shares[my - 1] (:179-185): the dealer's own (s', s)
      for (size_t p = 0; p < S; p++) {
        memcpy(own + 64 * p, sp_out + 32 * (p * n + js[p]), 32);
        memcpy(own + 64 * p + 32, s_out + 32 * (p * n + js[p]), 32);
      }
    return DKG_OK;
  });
}

// ---- hosted seats through rounds 3-5 (seat_finalise.hip)
namespace {

// The index arrays of one *_ceremonies call in one upload: x | party | crow | drow | 0, 1, 2, ..
struct CeremonyComplaintIndex {
  ComplaintIndex ix;
  std::vector<uint32_t> host;
  const uint32_t *x = nullptr, *party = nullptr, *crow = nullptr, *drow = nullptr, *seq = nullptr;
};
void upload_complaint_index(dkg_ctx* ctx, size_t n, size_t C, size_t items, const uint32_t* ceremony,
                            const uint32_t* accuser, const uint32_t* accused, CeremonyComplaintIndex& ci) {
  ci.ix = complaint_index(n, C, ceremony, accuser, accused);
  ci.host.resize(4 * C + items * C);
  memcpy(&ci.host[0], accuser, 4 * C);
  memcpy(&ci.host[C], ci.ix.party.data(), 4 * C);
  memcpy(&ci.host[2 * C], ci.ix.crow.data(), 4 * C);
  memcpy(&ci.host[3 * C], ci.ix.drow.data(), 4 * C);
  for (size_t k = 0; k < items * C; k++) ci.host[4 * C + k] = (uint32_t)k;
  uint32_t* d = buf<uint32_t>(ctx, "sc.idx", 4 * ci.host.size());
  h2d(ctx, d, ci.host.data(), 4 * ci.host.size());
  ci.x = d, ci.party = d + C, ci.crow = d + 2 * C, ci.drow = d + 3 * C, ci.seq = d + 4 * C;
}

// rows `rows` (0-based dealer rows) of src [..][N][32] behind one another into out
void gather_rows_host(const std::vector<uint32_t>& rows, size_t N, const uint8_t* src, uint8_t* out) {
  for (size_t r = 0; r < rows.size(); r++) memcpy(out + 32 * N * r, src + 32 * N * (size_t)rows[r], 32 * N);
}

}  // namespace

int dkg_complaints_verify_ceremonies(dkg_ctx* ctx, size_t B, size_t n, size_t t, size_t C, const uint32_t* ceremony,
                                     const uint32_t* accuser, const uint32_t* accused, const uint8_t* pk,
                                     const uint8_t* E, const uint8_t* fetched1, const uint8_t* enc,
                                     const uint8_t* proofs, int32_t* verdict, uint8_t* qualified) {
  return guarded(ctx, [&] {
    if (!B) return DKG_OK;
    const int rc0 = ceremony_args(ctx, n, t, {pk, E});
    if (rc0) return rc0;
    if (B > 0xffffffffu / n) return DKG_E_ARG;  // dealer rows are 32-bit
    if (!batch_complaint_args_ok(B, n, C, ceremony, accuser, accused, {enc, proofs, verdict})) return DKG_E_ARG;
    const size_t N = t + 1, V = B * n;
    hipStream_t st = ctx->stream;
    CeremonyComplaintIndex ci;  // the staging vectors live until the sync
    std::vector<uint8_t> hrows, hfet;
    int32_t* dver = nullptr;
    if (C) {
      upload_complaint_index(ctx, n, C, 1, ceremony, accuser, accused, ci);
      const size_t R = ci.ix.rows.size();
      hrows.resize(32 * R * N);
      gather_rows_host(ci.ix.rows, N, E, hrows.data());
      uint32_t* rc = buf<uint32_t>(ctx, "bp.rows2", 32 * R * N);
      h2d(ctx, rc, hrows.data(), 32 * R * N);
      const uint8_t* dfet = nullptr;
      if (fetched1) {  // by the commitment row's place, as k_cv_final reads it
        hfet.resize(R);
        for (size_t r = 0; r < R; r++) hfet[r] = fetched1[ci.ix.rows[r]];
        dfet = upload_mask(ctx, "sc.fetched1", hfet.data(), R);
      }
      uint32_t* dpk = buf<uint32_t>(ctx, "bp.pk", 32 * V);
      uint32_t* denc = buf<uint32_t>(ctx, "bp.enc", 128 * C);
      h2d(ctx, dpk, pk, 32 * V);
      h2d(ctx, denc, enc, 128 * C);
      dver = buf<int32_t>(ctx, "bp.verdict2", 4 * C);
      complaints2_rows(ctx, n, t, C, R, rc, ci.x, ci.party, ci.crow, ci.seq, dpk, denc, proofs, dfet, dver);
      check_launch(ctx);
      d2h(ctx, verdict, dver, 4 * C);
    }
    std::vector<uint8_t> rowok;
    if (qualified) {
      // the "row decodes" term needs every row: decoded for its validity only, in slabs of bounded size
      rowok.resize(V);
      const size_t slab = std::max<size_t>(1, ((size_t)1 << 18) / N);
      uint32_t* Ec = buf<uint32_t>(ctx, "sc.E", 32 * std::min(slab, V) * N);
      uint32_t* Eext = buf<uint32_t>(ctx, "sc.Eext", PTB * std::min(slab, V) * N);
      uint8_t* pok = buf<uint8_t>(ctx, "sc.pok", std::min(slab, V) * N);
      uint8_t* dok = buf<uint8_t>(ctx, "sc.rowok", V);
      for (size_t r0 = 0; r0 < V; r0 += slab) {
        const size_t rn = std::min(slab, V - r0);
        h2d(ctx, Ec, E + 32 * N * r0, 32 * N * rn);
        dkgk::decode_points(Ec, rn * N, Eext, rn * N, pok, st);
        dkgk::dealer_ok(rn, N, pok, dok + r0, st);
      }
      check_launch(ctx);
      d2h(ctx, rowok.data(), dok, V);
    }
    sync(ctx);
    if (qualified) {
      for (size_t i = 0; i < V; i++) qualified[i] = rowok[i] && (!fetched1 || fetched1[i]);
      for (size_t c = 0; c < C; c++)
        if (verdict[c] == 0) qualified[(size_t)ceremony[c] * n + accused[c] - 1] = 0;  // committee.rs:381-394
    }
    return DKG_OK;
  });
}

int dkg_complaints3_verify_ceremonies(dkg_ctx* ctx, size_t B, size_t n, size_t t, size_t C, const uint32_t* ceremony,
                                      const uint32_t* accuser, const uint32_t* accused, const uint8_t* share,
                                      const uint8_t* randomness, const uint8_t* E, const uint8_t* A,
                                      const uint8_t* qualified, const uint8_t* fetched3, int32_t* verdict,
                                      uint8_t* reconstruct) {
  return guarded(ctx, [&] {
    if (!B) return DKG_OK;
    const int rc0 = ceremony_args(ctx, n, t, {E, A});
    if (rc0) return rc0;
    if (B > 0xffffffffu / n) return DKG_E_ARG;
    if (!batch_complaint_args_ok(B, n, C, ceremony, accuser, accused, {share, randomness, verdict})) return DKG_E_ARG;
    const size_t N = t + 1, V = B * n;
    if (reconstruct) memset(reconstruct, 0, V);
    if (!C) return DKG_OK;
    CeremonyComplaintIndex ci;  // the staging vectors live until the sync
    upload_complaint_index(ctx, n, C, 2, ceremony, accuser, accused, ci);
    const size_t R = ci.ix.rows.size();
    std::vector<uint8_t> hrows(32 * 2 * R * N);  // the accused dealers' E rows, then their A rows
    gather_rows_host(ci.ix.rows, N, E, hrows.data());
    gather_rows_host(ci.ix.rows, N, A, hrows.data() + 32 * R * N);
    uint32_t* rc = buf<uint32_t>(ctx, "bp.rows4", 32 * 2 * R * N);
    h2d(ctx, rc, hrows.data(), 32 * 2 * R * N);
    const uint8_t* dq = upload_mask(ctx, "sc.qualified", qualified, V);
    const uint8_t* df3 = upload_mask(ctx, "sc.fetched3", fetched3, V);
    int32_t* dver = buf<int32_t>(ctx, "bp.verdict4", 4 * C);
    complaints4_rows(ctx, n, t, C, R, rc, ci.x, ci.crow, ci.drow, ci.seq, share, randomness, dq, df3, dver);
    check_launch(ctx);
    d2h(ctx, verdict, dver, 4 * C);
    sync(ctx);
    if (reconstruct)
      for (size_t c = 0; c < C; c++)  // committee.rs:643, :664-669
        if (verdict[c] == 0 || verdict[c] == DKG_COMPLAINT_NO_PHASE3)
          reconstruct[(size_t)ceremony[c] * n + accused[c] - 1] = 1;
    return DKG_OK;
  });
}

int dkg_party_round3_seats(dkg_ctx* ctx, size_t B, size_t n, size_t t, size_t S, const uint32_t* cer,
                           const uint32_t* js, const uint8_t* qualified, const uint8_t* s, uint8_t* final_share,
                           uint8_t* public_share) {
  (void)t;
  return guarded(ctx, [&] {
    if (!S) return DKG_OK;
    if (!B || !n || !cer || !js || !qualified || !s || !final_share) return DKG_E_ARG;
    if (B > 0xffffffffu / n || S >= 0xffffffffu) return DKG_E_ARG;
    for (size_t p = 0; p < S; p++)
      if (cer[p] >= B || js[p] >= n) return DKG_E_ARG;  // before any launch
    hipStream_t st = ctx->stream;
    const uint8_t* dq = upload_mask(ctx, "sr.q", qualified, B * n);
    uint32_t* dcer = buf<uint32_t>(ctx, "sr.cer", 4 * S);
    h2d(ctx, dcer, cer, 4 * S);
    const uint32_t* ds = upload_scalars(ctx, "sr.s", s, S * n);
    uint32_t* fs = buf<uint32_t>(ctx, "sr.fs", 32 * S);
    dkgk::seat_share_sum(S, n, dcer, dq, ds, fs, st);  // committee.rs:453-461
    d2h(ctx, final_share, fs, 32 * S);
    if (public_share) {  // :462-467
      uint32_t* ge = buf<uint32_t>(ctx, "sr.ge", PTB * S);
      uint32_t* oc = buf<uint32_t>(ctx, "sr.out", 32 * S);
      dkgk::fixed_base(S, fs, ctx->tab_gw, ge, st);
      dkgk::encode_points(ge, S, S, oc, st);
      d2h(ctx, public_share, oc, 32 * S);
    }
    check_launch(ctx);
    sync(ctx);
    return DKG_OK;
  });
}

int dkg_finalise_seats(dkg_ctx* ctx, size_t B, size_t n, size_t t, size_t S, const uint32_t* cer, const uint32_t* js,
                       const uint8_t* qualified, const uint8_t* reconstruct, const uint8_t* fetched3,
                       const uint8_t* r2_error, const uint8_t* r4_error, const uint8_t* A0, const uint8_t* s,
                       size_t D5, const uint32_t* d_ceremony, const uint32_t* d_sender, const uint32_t* d_dealer,
                       const uint8_t* d_share, uint8_t* mpk, int32_t* status, int32_t* recovery_index) {
  enum { SF_LAGRANGE, SF_MPK };
  static const PhaseRow SF_ROWS[] = {{"lagrange", 1u << SF_LAGRANGE}, {"mpk", 1u << SF_MPK}};
  return guarded(ctx, [&] {
    if (!S) return DKG_OK;
    if (!B || !n || !cer || !js || !qualified || !reconstruct || !A0 || !s || !mpk || !status) return DKG_E_ARG;
    if (D5 && (!d_ceremony || !d_sender || !d_dealer || !d_share)) return DKG_E_ARG;
    // party indices are multipliers below 2^24 on the device; rows, seats and list places are 32-bit
    if (n >= ((size_t)1 << 24) || B > 0xffffffffu / n || S >= 0xffffffffu || D5 >= 0xffffffffu) return DKG_E_ARG;
    for (size_t p = 0; p < S; p++)
      if (cer[p] >= B || js[p] >= n) return DKG_E_ARG;
    for (size_t d = 0; d < D5; d++)
      if (d_ceremony[d] >= B || d_sender[d] < 1 || d_sender[d] > n || d_dealer[d] < 1 || d_dealer[d] > n)
        return DKG_E_ARG;
    constexpr uint32_t NONE = dkgk::SEAT_ROW_NONE;
    // the ceremonies named, and per ceremony its final parties and one record per reconstructed dealer
    std::vector<uint32_t> cers, slot;
    dkgh::distinct_places(S, cer, cers, slot);
    const size_t Bd = cers.size(), D = Bd * n;
    std::unordered_map<uint32_t, uint32_t> slot_of;
    slot_of.reserve(2 * Bd);
    std::vector<uint8_t> fin(D);
    std::vector<uint32_t> rec(D, NONE), rptr(Bd + 1, 0), rdeal;
    for (size_t c = 0; c < Bd; c++) {
      slot_of[cers[c]] = (uint32_t)c;
      const uint8_t *q = qualified + (size_t)cers[c] * n, *r = reconstruct + (size_t)cers[c] * n;
      for (size_t i = 0; i < n; i++) {
        if (r[i] && !q[i]) {
          ctx->err = "finalise: only qualified members should be reconstructed (committee.rs:746-747 panics)";
          return DKG_E_ARG;
        }
        fin[c * n + i] = q[i] && !r[i];  // :733-739
        if (r[i]) {
          rec[c * n + i] = (uint32_t)rdeal.size();
          rdeal.push_back((uint32_t)i);
        }
      }
      rptr[c + 1] = (uint32_t)rdeal.size();
    }
    const size_t K = rdeal.size();
    // the disclosures the reference's loop reads (:763-775), in CSR form per record
    auto key = [&](uint32_t g, uint32_t sender0, uint32_t dealer0) { return ((uint64_t)g * n + sender0) * n + dealer0; };
    std::unordered_set<uint64_t> seen;
    seen.reserve(2 * D5);
    std::vector<uint32_t> dptr(K + 1, 0), keep(D5, NONE);
    for (size_t d = 0; d < D5; d++) {
      if (!seen.insert(key(d_ceremony[d], d_sender[d] - 1, d_dealer[d] - 1)).second) {
        ctx->err = "finalise: a (ceremony, sender, dealer) disclosure is listed twice";
        return DKG_E_ARG;
      }
      const auto it = slot_of.find(d_ceremony[d]);
      if (it == slot_of.end()) continue;  // a ceremony no seat names
      const size_t c = it->second;
      const uint32_t k = rec[c * n + d_dealer[d] - 1];
      if (k == NONE || !fin[c * n + d_sender[d] - 1]) continue;
      keep[d] = k;
      dptr[k + 1]++;
    }
    size_t longest = 0;
    for (size_t k = 0; k < K; k++) {
      longest = std::max<size_t>(longest, dptr[k + 1]);
      dptr[k + 1] += dptr[k];
    }
    if (longest + 1 > dkgk::SEAT_LAGRANGE_MAX_POINTS) {
      ctx->err = "finalise: more disclosures for one dealer than the interpolation stages";
      return DKG_E_ARG;
    }
    const size_t kept = dptr[K];
    std::vector<uint32_t> dx(std::max<size_t>(1, kept)), fill(dptr.begin(), dptr.end() - 1);
    std::vector<uint8_t> hy(32 * std::max<size_t>(1, kept));
    for (size_t d = 0; d < D5; d++) {
      if (keep[d] == NONE) continue;
      const size_t at = fill[keep[d]]++;
      dx[at] = d_sender[d];
      memcpy(&hy[32 * at], d_share + 32 * d, 32);
    }
    // dkg_seat_finalise_status per seat; a_ok (null at first: by fetched3 alone) [D] = A0 decodes
    std::vector<uint32_t> pts(n);
    std::vector<uint8_t> apres(n);
    auto seat_status = [&](size_t p, const uint8_t* a_ok, int32_t* index) {
      const size_t c = slot[p], g = cers[c];
      std::fill(pts.begin(), pts.end(), 0u);
      for (uint32_t k = rptr[c]; k < rptr[c + 1]; k++) {
        const bool self = fin[c * n + js[p]] && seen.count(key((uint32_t)g, js[p], rdeal[k]));
        pts[rdeal[k]] = 1 + (dptr[k + 1] - dptr[k]) - (self ? 1 : 0);  // the seat uses its own share (:754-761)
      }
      for (size_t i = 0; i < n; i++) apres[i] = (!fetched3 || fetched3[g * n + i]) && (!a_ok || a_ok[c * n + i]);
      return dkg_seat_finalise_status(n, t, js[p], qualified + g * n, reconstruct + g * n, apres.data(), pts.data(),
                                      r2_error && r2_error[p], r4_error && r4_error[p], index);
    };
    std::vector<uint8_t> skip(S);
    std::vector<uint32_t> sx(S), own(S, NONE);
    for (size_t p = 0; p < S; p++) {
      int32_t index;
      skip[p] = seat_status(p, nullptr, &index) != DKG_FIN_OK;
      sx[p] = js[p] + 1;
      if (!qualified[(size_t)cer[p] * n + js[p]]) own[p] = (uint32_t)(slot[p] * n + js[p]);  // its own A_p0 (:190)
    }
    hipStream_t st = ctx->stream;
    // ---- the interpolations, one workgroup per seat
    uint32_t* dslot = buf<uint32_t>(ctx, "sf.slot", 4 * S);
    uint32_t* dsx = buf<uint32_t>(ctx, "sf.sx", 4 * S);
    uint32_t* down = buf<uint32_t>(ctx, "sf.own", 4 * S);
    uint8_t* dskip = buf<uint8_t>(ctx, "sf.skip", S);
    uint32_t* drptr = buf<uint32_t>(ctx, "sf.rptr", 4 * (Bd + 1));
    uint32_t* drdeal = buf<uint32_t>(ctx, "sf.rdeal", 4 * K);
    uint32_t* ddptr = buf<uint32_t>(ctx, "sf.dptr", 4 * (K + 1));
    uint32_t* ddx = buf<uint32_t>(ctx, "sf.dx", 4 * dx.size());
    h2d(ctx, dslot, slot.data(), 4 * S);
    h2d(ctx, dsx, sx.data(), 4 * S);
    h2d(ctx, down, own.data(), 4 * S);
    h2d(ctx, dskip, skip.data(), S);
    h2d(ctx, drptr, rptr.data(), 4 * (Bd + 1));
    h2d(ctx, drdeal, rdeal.data(), 4 * K);
    h2d(ctx, ddptr, dptr.data(), 4 * (K + 1));
    h2d(ctx, ddx, dx.data(), 4 * dx.size());
    const uint32_t* ds = upload_scalars(ctx, "sf.s", s, S * n);
    const uint32_t* dy = upload_scalars(ctx, "sf.dy", hy.data(), hy.size() / 32);
    uint32_t* sigma = buf<uint32_t>(ctx, "sf.sigma", 32 * S);
    phase_mark_serial(ctx, "seats", -1);
    dkgk::seat_lagrange(S, n, dslot, dsx, dskip, drptr, drdeal, ddptr, ddx, dy, ds, longest + 1, sigma, st);
    phase_mark_serial(ctx, "seats", SF_LAGRANGE);
    // ---- mpk_p = sum of the A_i0 it adds + g sigma_p (:789-795): only the named ceremonies' rows
    std::vector<uint8_t> ha0(32 * D);
    for (size_t c = 0; c < Bd; c++) memcpy(&ha0[32 * c * n], A0 + 32 * (size_t)cers[c] * n, 32 * n);
    uint32_t* a0c = buf<uint32_t>(ctx, "sf.a0c", 32 * D);
    uint32_t* a0e = buf<uint32_t>(ctx, "sf.a0e", PTB * D);
    uint8_t* a0ok = buf<uint8_t>(ctx, "sf.a0ok", D);
    uint8_t* fm = buf<uint8_t>(ctx, "sf.fin", D);
    uint32_t* H = buf<uint32_t>(ctx, "sf.H", PTB * Bd);
    uint32_t* Hs = buf<uint32_t>(ctx, "sf.Hs", PTB * S);
    uint32_t* ownp = buf<uint32_t>(ctx, "sf.ownp", PTB * S);
    uint32_t* ge = buf<uint32_t>(ctx, "sf.ge", PTB * S);
    uint32_t* oc = buf<uint32_t>(ctx, "sf.out", 32 * S);
    h2d(ctx, a0c, ha0.data(), 32 * D);
    h2d(ctx, fm, fin.data(), D);
    dkgk::decode_points(a0c, D, a0e, D, a0ok, st);
    dkgk::sum_points(n, a0e, D, fm, H, Bd, 0, st, Bd);
    dkgk::seat_gather_points(S, dslot, H, Bd, Hs, S, st);
    dkgk::fill_identity(S, ownp, st);
    dkgk::seat_gather_points(S, down, a0e, D, ownp, S, st);
    dkgk::add_points(S, Hs, ownp, S, Hs, st);
    dkgk::fixed_base(S, sigma, ctx->tab_gw, ge, st);
    dkgk::add_points(S, ge, Hs, S, ge, st);
    dkgk::encode_points(ge, S, S, oc, st);
    phase_mark_serial(ctx, "seats", SF_MPK);
    check_launch(ctx);
    std::vector<uint8_t> okh(D), outh(32 * S);
    d2h(ctx, okh.data(), a0ok, D);
    d2h(ctx, outh.data(), oc, 32 * S);
    sync(ctx);
    phase_collect(ctx, "seats", SF_ROWS, std::size(SF_ROWS));
    memset(mpk, 0, 32 * S);
    for (size_t p = 0; p < S; p++) {
      int32_t index = -1;
      status[p] = seat_status(p, okh.data(), &index);
      if (recovery_index) recovery_index[p] = index;
      if (status[p] != DKG_FIN_OK) continue;
      if (own[p] != NONE && !okh[own[p]]) {
        ctx->err = "finalise: a disqualified seat's own A_0 commitment does not decode";
        return DKG_E_DECODE;
      }
      memcpy(mpk + 32 * p, &outh[32 * p], 32);
    }
    return DKG_OK;
  });
}

int dkg_complaints_verify(dkg_ctx* ctx, size_t n, size_t t, size_t C, const uint32_t* accuser, const uint32_t* accused,
                          const uint8_t* pk, const uint8_t* E, const uint8_t* fetched1, const uint8_t* enc,
                          const uint8_t* proofs, int32_t* verdict, uint8_t* qualified) {
  return guarded(ctx, [&] {
    const int rc = ceremony_args(ctx, n, t, {pk, E});
    if (rc) return rc;
    if (!complaint_args_ok(n, C, accuser, accused, {enc, proofs, verdict})) return DKG_E_ARG;
    const size_t N = t + 1;
    uint32_t* dpk = buf<uint32_t>(ctx, "cv_pk", 32 * n);
    uint32_t* Ec = buf<uint32_t>(ctx, "cv_E", 32 * n * N);
    h2d(ctx, dpk, pk, 32 * n);
    h2d(ctx, Ec, E, 32 * n * N);
    std::vector<uint8_t> rowok(n);
    complaints_verify_core(ctx, n, t, C, accuser, accused, dpk, Ec, fetched1, enc, proofs, verdict, rowok.data());
    if (qualified) {
      for (size_t i = 0; i < n; i++) qualified[i] = rowok[i] && (!fetched1 || fetched1[i]);
      for (size_t c = 0; c < C; c++)
        if (verdict[c] == 0) qualified[accused[c] - 1] = 0;  // committee.rs:381-394: cleared only on Ok
    }
    return DKG_OK;
  });
}

int dkg_ceremony_verify_full_complaints(dkg_ctx* ctx, size_t n, size_t t, const uint8_t* E, const uint8_t* A,
                                        const uint8_t* e1, const uint8_t* ct, const uint8_t* sk, const uint8_t* pk,
                                        size_t C, const uint32_t* accuser, const uint32_t* accused,
                                        const uint8_t* proofs, dkg_ceremony_out* out, int32_t* verdict,
                                        int32_t* dissent) {
  return guarded(ctx, [&] {
    const int rc = ceremony_args(ctx, n, t, {out, E, A, e1, ct, sk, pk});
    if (rc) return rc;
    if (!complaint_args_ok(n, C, accuser, accused, {proofs, verdict})) return DKG_E_ARG;
    const Complaints2 c2{pk, C, accuser, accused, proofs, verdict, dissent};
    CeremonyInput in;
    in.E = E, in.A = A, in.e1 = e1, in.ct = ct, in.sk = sk, in.c2 = &c2;
    return verify_ceremony(ctx, n, t, in, out);
  });
}

// ---- round-4 complaints as a device batch, and the ceremonies that reconstruct by them
int dkg_complaints3_verify(dkg_ctx* ctx, size_t n, size_t t, size_t C, const uint32_t* accuser, const uint32_t* accused,
                           const uint8_t* share, const uint8_t* randomness, const uint8_t* E, const uint8_t* A,
                           const uint8_t* qualified, const uint8_t* fetched3, int32_t* verdict, uint8_t* reconstruct) {
  return guarded(ctx, [&] {
    const int rc = ceremony_args(ctx, n, t, {E, A});
    if (rc) return rc;
    if (!complaint_args_ok(n, C, accuser, accused, {share, randomness, verdict})) return DKG_E_ARG;
    const Commitments cm = upload_commitments(ctx, n, t + 1, E, A);
    complaints3_core(ctx, n, t, C, accuser, accused, share, randomness, cm.E, qualified, fetched3, verdict, nullptr);
    if (reconstruct) {
      const std::vector<uint8_t> p = proven_round4(n, C, accused, verdict);
      memcpy(reconstruct, p.data(), n);
    }
    return DKG_OK;
  });
}

int dkg_ceremony_verify_fetched_proven(dkg_ctx* ctx, size_t n, size_t t, const uint8_t* E, const uint8_t* A,
                                       const uint8_t* s, const uint8_t* s_prime, const uint8_t* fetched1,
                                       const uint8_t* fetched3, size_t C4, const uint32_t* accuser4,
                                       const uint32_t* accused4, const uint8_t* share4, const uint8_t* randomness4,
                                       dkg_ceremony_out* out, int32_t* verdict4, int32_t* finalise_status,
                                       int32_t* recovery_index) {
  return guarded(ctx, [&] {
    const int rc = ceremony_args(ctx, n, t, {out, E, A, s, s_prime, fetched1, fetched3});
    if (rc) return rc;
    if (!complaint_args_ok(n, C4, accuser4, accused4, {share4, randomness4, verdict4})) return DKG_E_ARG;
    const Complaints4 c4{C4, accuser4, accused4, share4, randomness4, verdict4, finalise_status, recovery_index};
    CeremonyInput in;
    in.E = E, in.A = A, in.s = s, in.s_prime = s_prime, in.fetched1 = fetched1, in.fetched3 = fetched3, in.c4 = &c4;
    return verify_ceremony(ctx, n, t, in, out);
  });
}

int dkg_ceremony_verify_full_proven(dkg_ctx* ctx, size_t n, size_t t, const uint8_t* E, const uint8_t* A,
                                    const uint8_t* e1, const uint8_t* ct, const uint8_t* sk, const uint8_t* pk,
                                    size_t C, const uint32_t* accuser, const uint32_t* accused, const uint8_t* proofs,
                                    const uint8_t* fetched3, size_t C4, const uint32_t* accuser4,
                                    const uint32_t* accused4, const uint8_t* share4, const uint8_t* randomness4,
                                    dkg_ceremony_out* out, int32_t* verdict, int32_t* dissent, int32_t* verdict4,
                                    int32_t* finalise_status, int32_t* recovery_index) {
  return guarded(ctx, [&] {
    const int rc = ceremony_args(ctx, n, t, {out, E, A, e1, ct, sk, pk});
    if (rc) return rc;
    if (!complaint_args_ok(n, C, accuser, accused, {proofs, verdict}) ||
        !complaint_args_ok(n, C4, accuser4, accused4, {share4, randomness4, verdict4}))
      return DKG_E_ARG;
    const Complaints2 c2{pk, C, accuser, accused, proofs, verdict, dissent};
    const Complaints4 c4{C4, accuser4, accused4, share4, randomness4, verdict4, finalise_status, recovery_index};
    CeremonyInput in;
    in.E = E, in.A = A, in.e1 = e1, in.ct = ct, in.sk = sk, in.fetched3 = fetched3, in.c2 = &c2, in.c4 = &c4;
    return verify_ceremony(ctx, n, t, in, out);
  });
}


// ---- full mode for batches of ceremonies (hybrid_batch.hip)
int dkg_ctx_set_batch_full_chunk(dkg_ctx* ctx, size_t ceremonies) {
  if (!ctx) return DKG_E_ARG;
  ctx->bfull_chunk = ceremonies;
  return DKG_OK;
}

int dkg_member_keys_batch(dkg_ctx* ctx, const uint8_t master[32], uint32_t ceremony0, size_t B, size_t n,
                          uint8_t* sk_out, uint8_t* pk_out) {
  return guarded(ctx, [&] {
    if (!master || !sk_out || !pk_out) return DKG_E_ARG;
    const size_t V = B * n;
    if (!V) return DKG_OK;
    static const char tag[] = "dkg-amd/v1/member";
    std::vector<uint8_t> sk(32 * V), pk(32 * V);
    for (size_t c = 0; c < B; c++) {
      const uint32_t ceremony = ceremony0 + (uint32_t)c;
      for (size_t j = 0; j < n; j++) {  // MemberCommunicationKey::new (procedure_keys.rs:72-76), as dkg_member_keys
        uint8_t msg[sizeof tag - 1 + 40], seed[32], st[64];
        memcpy(msg, tag, sizeof tag - 1);
        memcpy(msg + sizeof tag - 1, master, 32);
        for (int k = 0; k < 4; k++) {
          msg[sizeof tag - 1 + 32 + k] = (uint8_t)(ceremony >> (8 * k));
          msg[sizeof tag - 1 + 36 + k] = (uint8_t)((uint32_t)j >> (8 * k));
        }
        dkgh::blake2b(seed, 32, msg, sizeof msg);
        dkgh::chacha20(seed, 0, st, 64);
        dkgh::zl_to_bytes(&sk[32 * (c * n + j)], dkgh::zl_from_bytes_wide(st, 64));
      }
    }
    uint32_t* dsk = buf<uint32_t>(ctx, "mk_sk", 32 * V);
    uint32_t* dpe = buf<uint32_t>(ctx, "mk_pk_ext", PTB * V);
    uint32_t* dpc = buf<uint32_t>(ctx, "mk_pk", 32 * V);
    h2d(ctx, dsk, sk.data(), 32 * V);
    dkgk::fixed_base(V, dsk, ctx->tab_gw, dpe, ctx->stream);  // to_public of all B*n keys, one launch
    dkgk::encode_points(dpe, V, V, dpc, ctx->stream);
    check_launch(ctx);
    d2h(ctx, pk.data(), dpc, 32 * V);
    sync(ctx);
    // committee.rs:134-135: each ceremony's keys sorted by public-key bytes
    std::vector<size_t> order(n);
    for (size_t c = 0; c < B; c++) {
      const uint8_t* cpk = &pk[32 * c * n];
      for (size_t j = 0; j < n; j++) order[j] = j;
      std::sort(order.begin(), order.end(),
                [&](size_t a, size_t b) { return memcmp(cpk + 32 * a, cpk + 32 * b, 32) < 0; });
      for (size_t q = 0; q < n; q++) {
        memcpy(sk_out + 32 * (c * n + q), &sk[32 * (c * n + order[q])], 32);
        memcpy(pk_out + 32 * (c * n + q), cpk + 32 * order[q], 32);
      }
    }
    return DKG_OK;
  });
}

int dkg_encrypt_shares_batch(dkg_ctx* ctx, size_t B, size_t n, const uint8_t* pk, const uint8_t* s,
                             const uint8_t* s_prime, const uint8_t* r, uint8_t* e1, uint8_t* ct) {
  return guarded(ctx, [&] {
    if (!pk || !s || !s_prime || !r || !e1 || !ct) return DKG_E_ARG;
    if (!B || !n) return DKG_OK;
    const size_t V = B * n, items = 2 * V * n;
    uint32_t* dpk = buf<uint32_t>(ctx, "bx_pk", 32 * V);
    h2d(ctx, dpk, pk, 32 * V);
    uint32_t* ds = upload_scalars(ctx, "bx_s", s, V * n);
    uint32_t* dsp = upload_scalars(ctx, "bx_sp", s_prime, V * n);
    uint32_t* dr = upload_scalars(ctx, "bx_r", r, items);
    uint32_t* de1 = buf<uint32_t>(ctx, "bx_e1", 32 * items);
    uint32_t* dct = buf<uint32_t>(ctx, "bx_ct", 32 * items);
    uint8_t* pok = buf<uint8_t>(ctx, "bx_pkok", V);
    uint8_t* ok = hbuf<uint8_t>(ctx, "hb.bf_pkok", V);
    encrypt_batch_device(ctx, B, n, dpk, ds, dsp, dr, de1, dct, pok);
    d2h(ctx, ok, pok, V);
    d2h(ctx, e1, de1, 32 * items);
    d2h(ctx, ct, dct, 32 * items);
    sync(ctx);
    phase_collect(ctx, "bfull", BF_ROWS, BF_PHASES);
    return batch_keys_status(ctx, ok, V);
  });
}

int dkg_decrypt_shares_batch(dkg_ctx* ctx, size_t B, size_t n, const uint8_t* sk, const uint8_t* e1, const uint8_t* ct,
                             uint8_t* s, uint8_t* s_prime, uint8_t* ok) {
  return guarded(ctx, [&] {
    if (!sk || !e1 || !ct || !s || !s_prime) return DKG_E_ARG;
    if (!B || !n) return DKG_OK;
    const size_t V = B * n, items = 2 * V * n;
    uint32_t* dsk = upload_scalars(ctx, "bx_sk", sk, V);
    uint32_t* de1 = buf<uint32_t>(ctx, "bx_e1", 32 * items);
    uint32_t* dct = buf<uint32_t>(ctx, "bx_ct", 32 * items);
    h2d(ctx, de1, e1, 32 * items);
    h2d(ctx, dct, ct, 32 * items);
    uint32_t* ds = buf<uint32_t>(ctx, "bx_s", 32 * V * n);
    uint32_t* dsp = buf<uint32_t>(ctx, "bx_sp", 32 * V * n);
    uint8_t* iok = buf<uint8_t>(ctx, "bx_ok", items);
    decrypt_batch_device(ctx, B, n, dsk, de1, dct, ds, dsp, iok, nullptr);
    d2h(ctx, s, ds, 32 * V * n);
    d2h(ctx, s_prime, dsp, 32 * V * n);
    if (ok) d2h(ctx, ok, iok, items);
    sync(ctx);
    phase_collect(ctx, "bfull", BF_ROWS, BF_PHASES);
    return DKG_OK;
  });
}

// Full-mode batch: round 1 of every ceremony with its shares hybrid-encrypted to that ceremony's sorted
// member keys, the receivers' decryption, then rounds 2-5 on the decrypted shares as the plaintext
// batch runs them.  The hybrid stage is serialised on the ctx stream: the encryption in ms_round1, the
// decryption in ms_checks.
int dkg_ceremony_batch_full_device(dkg_ctx* ctx, size_t B, size_t n, size_t t, const void* d_a, const void* d_b,
                                   const void* d_r, const uint8_t* sk, const uint8_t* pk, dkg_batch_out* out) {
  return guarded(ctx, [&] {
    const int rc = ceremony_args(ctx, n, t, {out, sk, pk});
    if (rc || !B) return rc;
    if (!d_a || !d_b || !d_r) return DKG_E_ARG;
    const size_t N = t + 1, V = B * n, items = 2 * V * n;
    uint32_t* dsk = upload_scalars(ctx, "bfm_sk", sk, V);
    uint32_t* dpk = buf<uint32_t>(ctx, "bfm_pk", 32 * V);
    h2d(ctx, dpk, pk, 32 * V);
    HCK(hipEventRecord(ctx->ev[0], ctx->stream));
    uint32_t* Ec = buf<uint32_t>(ctx, "bat_E", 32 * V * N);
    uint32_t* Ac = buf<uint32_t>(ctx, "bat_A", 32 * V * N);
    uint32_t* ds = buf<uint32_t>(ctx, "bat_s", 32 * V * n);
    uint32_t* dsp = buf<uint32_t>(ctx, "bat_sp", 32 * V * n);
    uint32_t* e1 = buf<uint32_t>(ctx, "bfm_e1", 32 * items);
    uint32_t* ct = buf<uint32_t>(ctx, "bfm_ct", 32 * items);
    uint32_t* rs = buf<uint32_t>(ctx, "bfm_s", 32 * V * n);
    uint32_t* rsp = buf<uint32_t>(ctx, "bfm_sp", 32 * V * n);
    uint8_t* iok = buf<uint8_t>(ctx, "bfm_iok", items);
    uint8_t* eok = buf<uint8_t>(ctx, "bfm_eok", V);
    uint8_t* pok = buf<uint8_t>(ctx, "bfm_pkok", V);
    uint8_t* ok = hbuf<uint8_t>(ctx, "hb.bf_pkok", V);  // pinned: the copy below must not stall the queue
    BatchRound1 r1(ctx, V, n, t, (const uint32_t*)d_a, (const uint32_t*)d_b, ds, dsp);
    wait_shares(ctx, ctx->stream);  // the encryption reads the shares the side stream evaluates
    encrypt_batch_device(ctx, B, n, dpk, ds, dsp, (const uint32_t*)d_r, e1, ct, pok);  // committee.rs:169-172
    d2h(ctx, ok, pok, V);
    HCK(hipEventRecord(ctx->ev[1], ctx->stream));
    decrypt_batch_device(ctx, B, n, dsk, e1, ct, rs, rsp, iok, eok);                    // committee.rs:282-286
    std::unique_ptr<ExtScope> ext(r1.deferred() ? nullptr : new ExtScope(ctx, V, N));
    batch_receivers(ctx, B, n, t, Ec, Ac, rs, rsp, out, eok);
    phase_collect(ctx, "bfull", BF_ROWS, BF_PHASES);
    batch_times(ctx, out, true);
    return batch_keys_status(ctx, ok, V);
  });
}

int dkg_ceremony_batch_verify_full(dkg_ctx* ctx, size_t B, size_t n, size_t t, const uint8_t* E, const uint8_t* A,
                                   const uint8_t* e1, const uint8_t* ct, const uint8_t* sk, dkg_batch_out* out,
                                   uint8_t* s_out, uint8_t* s_prime_out) {
  return guarded(ctx, [&] {
    const int rc = ceremony_args(ctx, n, t, {out, E, A, e1, ct, sk});
    if (rc || !B) return rc;
    BatchInput in;
    in.E = E, in.A = A, in.e1 = e1, in.ct = ct, in.sk = sk, in.s_out = s_out, in.s_prime_out = s_prime_out;
    return verify_batch(ctx, B, n, t, in, out);
  });
}

// ---- batches that decide by the proven complaints (batch_complaints, batch_proven_outcome)
int dkg_ceremony_batch_verify_proven(dkg_ctx* ctx, size_t B, size_t n, size_t t, const uint8_t* E, const uint8_t* A,
                                     const uint8_t* s, const uint8_t* s_prime, const uint8_t* fetched1,
                                     const uint8_t* fetched3, size_t C4, const uint32_t* ceremony4,
                                     const uint32_t* accuser4, const uint32_t* accused4, const uint8_t* share4,
                                     const uint8_t* randomness4, dkg_batch_out* out, int32_t* verdict4,
                                     int32_t* finalise_status, int32_t* recovery_index) {
  return guarded(ctx, [&] {
    const int rc = ceremony_args(ctx, n, t, {out, E, A, s, s_prime});
    if (rc || !B) return rc;
    if (B * n >= ((size_t)1 << 31) ||
        !batch_complaint_args_ok(B, n, C4, ceremony4, accuser4, accused4, {share4, randomness4, verdict4}))
      return DKG_E_ARG;
    const BatchComplaints4 c4{C4, ceremony4, accuser4, accused4, share4, randomness4, verdict4, finalise_status,
                              recovery_index};
    BatchInput in;
    in.E = E, in.A = A, in.s = s, in.s_prime = s_prime, in.fetched1 = fetched1, in.fetched3 = fetched3, in.c4 = &c4;
    return verify_batch(ctx, B, n, t, in, out);
  });
}

int dkg_ceremony_batch_verify_full_proven(dkg_ctx* ctx, size_t B, size_t n, size_t t, const uint8_t* E,
                                          const uint8_t* A, const uint8_t* e1, const uint8_t* ct, const uint8_t* sk,
                                          const uint8_t* pk, size_t C, const uint32_t* ceremony,
                                          const uint32_t* accuser, const uint32_t* accused, const uint8_t* proofs,
                                          const uint8_t* fetched3, size_t C4, const uint32_t* ceremony4,
                                          const uint32_t* accuser4, const uint32_t* accused4, const uint8_t* share4,
                                          const uint8_t* randomness4, dkg_batch_out* out, uint8_t* s_out,
                                          uint8_t* s_prime_out, int32_t* verdict, int32_t* dissent, int32_t* verdict4,
                                          int32_t* finalise_status, int32_t* recovery_index) {
  return guarded(ctx, [&] {
    const int rc = ceremony_args(ctx, n, t, {out, E, A, e1, ct, sk, pk});
    if (rc || !B) return rc;
    if (B * n >= ((size_t)1 << 31) ||
        !batch_complaint_args_ok(B, n, C, ceremony, accuser, accused, {proofs, verdict}) ||
        !batch_complaint_args_ok(B, n, C4, ceremony4, accuser4, accused4, {share4, randomness4, verdict4}))
      return DKG_E_ARG;
    const BatchComplaints2 c2{pk, C, ceremony, accuser, accused, proofs, verdict, dissent};
    const BatchComplaints4 c4{C4, ceremony4, accuser4, accused4, share4, randomness4, verdict4, finalise_status,
                              recovery_index};
    BatchInput in;
    in.E = E, in.A = A, in.e1 = e1, in.ct = ct, in.sk = sk, in.fetched3 = fetched3, in.c2 = &c2, in.c4 = &c4;
    in.s_out = s_out, in.s_prime_out = s_prime_out;
    return verify_batch(ctx, B, n, t, in, out);
  });
}

int dkg_misbehaviour_prove(dkg_ctx* ctx, size_t B, const uint8_t* sk, const uint8_t* enc, const uint8_t* w,
                           uint8_t* proofs) {
  return guarded(ctx, [&] {
    if (!sk || !enc || !w || !proofs) return DKG_E_ARG;
    if (!B) return DKG_OK;
    // per complaint 7 single-term products: K_share, K_rand, pk, and the two DLEQ announcements
    std::vector<uint8_t> sc, pt, out(32 * 7 * B);
    for (size_t b = 0; b < B; b++) {
      const uint8_t *e1r = enc + 128 * b, *e1s = e1r + 64, *x = sk + 32 * b, *w1 = w + 64 * b, *w2 = w1 + 32;
      const uint8_t* P[7] = {e1s, e1r, BASEPOINT, BASEPOINT, e1s, BASEPOINT, e1r};
      const uint8_t* S[7] = {x, x, x, w1, w1, w2, w2};
      for (int k = 0; k < 7; k++) {
        put32(pt, P[k]);
        put32(sc, S[k]);
      }
    }
    std::vector<uint8_t> ok;
    msm_host(ctx, 7 * B, 1, sc.data(), pt.data(), out.data(), ok);
    for (size_t b = 0; b < B; b++) {
      for (int k = 0; k < 7; k++)
        if (!ok[7 * b + k]) {
          ctx->err = "misbehaviour_prove: a ciphertext point does not decode";
          return DKG_E_DECODE;
        }
      const uint8_t *o = &out[32 * 7 * b], *e1r = enc + 128 * b, *e1s = e1r + 64;
      const uint8_t *Ks = o, *Kr = o + 32, *pk = o + 64;
      uint8_t* p = proofs + 192 * b;
      memcpy(p, Ks, 32);       // share_key      (broadcast.rs:197-199, recover_symmetric_key)
      memcpy(p + 32, Kr, 32);  // randomness_key (:200-202)
      const dkgh::Zl x = zl32(sk + 32 * b);
      // CorrectHybridDecrKeyZkp = DLEQ(g, e1, pk, K; sk) (correct_hybrid_decryption_key/zkp.rs:27-47)
      dkgh::Zl c1 = dleq_challenge(BASEPOINT, e1s, pk, Ks, o + 96, o + 128);
      dkgh::Zl r1 = dkgh::zl_add(dkgh::zl_mul(c1, x), zl32(w + 64 * b));
      dkgh::Zl c2 = dleq_challenge(BASEPOINT, e1r, pk, Kr, o + 160, o + 192);
      dkgh::Zl r2 = dkgh::zl_add(dkgh::zl_mul(c2, x), zl32(w + 64 * b + 32));
      dkgh::zl_to_bytes(p + 64, c1);
      dkgh::zl_to_bytes(p + 96, r1);
      dkgh::zl_to_bytes(p + 128, c2);
      dkgh::zl_to_bytes(p + 160, r2);
    }
    return DKG_OK;
  });
}

int dkg_complaint1_verify(dkg_ctx* ctx, size_t B, size_t t, const uint32_t* accuser, const uint8_t* pk,
                          const uint8_t* enc, const uint8_t* E, const uint8_t* proofs, int32_t* result) {
  return guarded(ctx, [&] {
    int rc = need_env(ctx);
    if (rc) return rc;
    if (!accuser || !pk || !enc || !E || !proofs || !result) return DKG_E_ARG;
    if (!B) return DKG_OK;
    const size_t N = t + 1;
    // phase A, 6 two-term MSMs per complaint: both DLEQ announcements of both proofs
    // (dl_equality/zkp.rs:60-63) and the two h/g combinations of the decrypted scalars
    std::vector<uint8_t> sc, pt, outA(32 * 6 * B), sb, pb, outB(32 * B);
    for (size_t b = 0; b < B; b++) {
      const uint8_t *e1r = enc + 128 * b, *ctr = e1r + 32, *e1s = e1r + 64, *cts = e1r + 96;
      const uint8_t *P = proofs + 192 * b, *Ks = P, *Kr = P + 32, *pkb = pk + 32 * b;
      const dkgh::Zl zero = dkgh::zl_from_u64(0);
      const dkgh::Zl nc1 = dkgh::zl_sub(zero, zl32(P + 64)), nc2 = dkgh::zl_sub(zero, zl32(P + 128));
      const dkgh::Zl p1 = sym_scalar(Ks, cts), p2 = sym_scalar(Kr, ctr);  // share, randomness
      put32(sc, P + 96); putzl(sc, nc1); put32(pt, BASEPOINT); put32(pt, pkb);   // a1 = g r1 - pk c1
      put32(sc, P + 96); putzl(sc, nc1); put32(pt, e1s); put32(pt, Ks);          // a2 = e1 r1 - K c1
      put32(sc, P + 160); putzl(sc, nc2); put32(pt, BASEPOINT); put32(pt, pkb);
      put32(sc, P + 160); putzl(sc, nc2); put32(pt, e1r); put32(pt, Kr);
      putzl(sc, p1); putzl(sc, p2); put32(pt, ctx->h); put32(pt, BASEPOINT);  // quirk: h*share + g*rand
      putzl(sc, p2); putzl(sc, p1); put32(pt, ctx->h); put32(pt, BASEPOINT);  // accusation: h*rand + g*share
      std::vector<uint8_t> pw = index_powers(accuser[b], N);
      sb.insert(sb.end(), pw.begin(), pw.end());
      pb.insert(pb.end(), E + 32 * N * b, E + 32 * N * (b + 1));
    }
    std::vector<uint8_t> okA, okB;
    msm_host(ctx, 6 * B, 2, sc.data(), pt.data(), outA.data(), okA);
    msm_host(ctx, B, N, sb.data(), pb.data(), outB.data(), okB);  // sum_k j^k E_k
    for (size_t b = 0; b < B; b++) {
      bool ok = okB[b];
      for (int k = 0; k < 6; k++) ok = ok && okA[6 * b + k];
      if (!ok) {
        result[b] = -1;
        continue;
      }
      const uint8_t *e1r = enc + 128 * b, *e1s = e1r + 64, *P = proofs + 192 * b, *o = &outA[32 * 6 * b];
      uint8_t c[32];
      dkgh::zl_to_bytes(c, dleq_challenge(BASEPOINT, e1s, pk + 32 * b, P, o, o + 32));
      const bool v1 = memcmp(c, P + 64, 32) == 0;
      dkgh::zl_to_bytes(c, dleq_challenge(BASEPOINT, e1r, pk + 32 * b, P + 32, o + 64, o + 96));
      const bool v2 = memcmp(c, P + 128, 32) == 0;
      const uint8_t* rhs = &outB[32 * b];
      if (!v1 || !v2) result[b] = 1;                            // InvalidProofOfMisbehaviour
      else if (memcmp(o + 128, rhs, 32) == 0) result[b] = 1;   // ProofOfMisbehaviour::verify quirk (:271-283)
      else if (memcmp(o + 160, rhs, 32) == 0) result[b] = 2;   // FalseClaimedInequality (broadcast.rs:94-96)
      else result[b] = 0;
    }
    return DKG_OK;
  });
}

int dkg_complaint3_verify(dkg_ctx* ctx, size_t B, size_t t, const uint32_t* accuser, const uint8_t* share,
                          const uint8_t* randomness, const uint8_t* E, const uint8_t* A, int32_t* result) {
  return guarded(ctx, [&] {
    int rc = need_env(ctx);
    if (rc) return rc;
    if (!accuser || !share || !randomness || !E || !A || !result) return DKG_E_ARG;
    if (!B) return DKG_OK;
    const size_t N = t + 1;
    std::vector<uint8_t> sc, pt, outA(32 * 2 * B), sb, pb, outB(32 * 2 * B);
    const uint8_t zero[32] = {0};
    for (size_t b = 0; b < B; b++) {
      put32(sc, share + 32 * b); put32(sc, randomness + 32 * b); put32(pt, BASEPOINT); put32(pt, ctx->h);
      put32(sc, share + 32 * b); put32(sc, zero); put32(pt, BASEPOINT); put32(pt, BASEPOINT);
      std::vector<uint8_t> pw = index_powers(accuser[b], N);
      for (int r = 0; r < 2; r++) {
        sb.insert(sb.end(), pw.begin(), pw.end());
        const uint8_t* C = r == 0 ? E : A;
        pb.insert(pb.end(), C + 32 * N * b, C + 32 * N * (b + 1));
      }
    }
    std::vector<uint8_t> okA, okB;
    msm_host(ctx, 2 * B, 2, sc.data(), pt.data(), outA.data(), okA);
    msm_host(ctx, 2 * B, N, sb.data(), pb.data(), outB.data(), okB);
    for (size_t b = 0; b < B; b++) {
      if (!(okA[2 * b] && okA[2 * b + 1] && okB[2 * b] && okB[2 * b + 1])) {
        result[b] = -1;
        continue;
      }
      const uint8_t *pass = &outA[64 * b], *fail = pass + 32, *rE = &outB[64 * b], *rA = rE + 32;
      if (memcmp(pass, rE, 32) != 0) result[b] = 3;       // FalseClaimedEquality (broadcast.rs:129-130)
      else if (memcmp(fail, rA, 32) == 0) result[b] = 2;  // FalseClaimedInequality (:131-132)
      else result[b] = 0;
    }
    return DKG_OK;
  });
}

int dkg_dealer_coeffs(const uint8_t master[32], uint32_t ceremony, size_t d0, size_t D, size_t t, uint8_t* a,
                      uint8_t* b) {
  if (!master || (!a && !b)) return DKG_E_ARG;
  const size_t N = t + 1;
  static const char tag[] = "dkg-amd/v1/dealer";
  std::vector<uint8_t> stream(2 * N * 64);
  for (size_t i = 0; i < D; i++) {
    uint8_t msg[sizeof tag - 1 + 40];
    memcpy(msg, tag, sizeof tag - 1);
    memcpy(msg + sizeof tag - 1, master, 32);
    const uint32_t dealer = (uint32_t)(d0 + i);
    for (int k = 0; k < 4; k++) {
      msg[sizeof tag - 1 + 32 + k] = (uint8_t)(ceremony >> (8 * k));
      msg[sizeof tag - 1 + 36 + k] = (uint8_t)(dealer >> (8 * k));
    }
    uint8_t seed[32];
    dkgh::blake2b(seed, 32, msg, sizeof msg);
    dkgh::chacha20(seed, 0, stream.data(), stream.size());
    for (size_t k = 0; k < N; k++) {  // hiding polynomial first (committee.rs:143-146)
      if (b) dkgh::zl_to_bytes(b + 32 * (i * N + k), dkgh::zl_from_bytes_wide(&stream[64 * k], 64));
      if (a) dkgh::zl_to_bytes(a + 32 * (i * N + k), dkgh::zl_from_bytes_wide(&stream[64 * (N + k)], 64));
    }
  }
  return DKG_OK;
}

}  // extern "C"
