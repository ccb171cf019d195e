// dkg_receiver_plan_for: how one party's evaluations P_i(x) = sum_k x^k C_i[k] are cut into chunks
// and folded (receivers.hip runs exactly this plan).  Host only, a pure function of (n, t, x, chunk).
#include <algorithm>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "../../include/dkg_amd.h"
#include "host_crypto.h"

namespace dkgh {

// NAF of a 256-bit little-endian value: +1 / -1 digit bits in pos / neg (8 words each); returns the
// length (0 for zero; the top digit is +1 at length - 1, which is <= 255 for a value < 2^255).
int naf256(const uint8_t v[32], uint32_t pos[8], uint32_t neg[8], int* weight) {
  uint32_t w[9] = {0};
  for (int i = 0; i < 32; i++) w[i / 4] |= (uint32_t)v[i] << (8 * (i % 4));
  memset(pos, 0, 32);
  memset(neg, 0, 32);
  int len = 0, wt = 0;
  for (int i = 0; i < 257; i++) {
    bool any = false;
    for (int k = 0; k < 9; k++) any |= w[k] != 0;
    if (!any) break;
    if (w[0] & 1u) {
      wt++;
      if ((w[0] & 3u) == 1u) {
        if (i < 256) pos[i / 32] |= 1u << (i % 32);
        w[0] -= 1;  // the low bit is set: no borrow
      } else {
        if (i < 256) neg[i / 32] |= 1u << (i % 32);
        for (int k = 0; k < 9 && ++w[k] == 0; k++) {}
      }
      len = i + 1;
    }
    for (int k = 0; k < 8; k++) w[k] = (w[k] >> 1) | (w[k + 1] << 31);
    w[8] >>= 1;
  }
  if (weight) *weight = wt;
  return len;
}

// The distinct values of v[0 .. count) in order of first appearance, and place[p] = the position of v[p]
// among them: the item lists of the pair evaluation (distinct rows to decode, distinct indices to plan).
void distinct_places(size_t count, const uint32_t* v, std::vector<uint32_t>& distinct, std::vector<uint32_t>& place) {
  distinct.clear();
  place.resize(count);
  std::unordered_map<uint32_t, uint32_t> at;
  for (size_t p = 0; p < count; p++) {
    auto it = at.find(v[p]);
    if (it == at.end()) {
      it = at.emplace(v[p], (uint32_t)distinct.size()).first;
      distinct.push_back(v[p]);
    }
    place[p] = it->second;
  }
}

}  // namespace dkgh

namespace {

using dkgh::naf256;

// doublings + additions of the signed-digit chain of multiplier m (1: none)
int chain_ops(const uint8_t m[32]) {
  uint32_t p[8], q[8];
  int wt = 0;
  const int len = naf256(m, p, q, &wt);
  return len <= 1 ? 0 : (len - 1) + (wt - 1);
}

void u32_bytes(uint8_t out[32], uint32_t x) {
  memset(out, 0, 32);
  for (int i = 0; i < 4; i++) out[i] = (uint8_t)(x >> (8 * i));
}

// The plan's multipliers for a forced chunk; false if it needs more than 16 stages.
bool fill_plan(size_t N, uint32_t x, size_t L, dkg_receiver_plan* out) {
  memset(out, 0, sizeof *out);
  if (L >= N) {  // one chunk: the serial walk
    out->chunk = (uint32_t)(L > 0xffffffffu ? 0xffffffffu : L);
    return true;
  }
  out->chunk = (uint32_t)L;
  dkgh::Zl y = dkgh::zl_from_u64(1);
  const dkgh::Zl xz = dkgh::zl_from_u64(x);
  for (size_t k = 0; k < L; k++) y = dkgh::zl_mul(y, xz);  // x^L: the integer itself while below l
  size_t G = (N + L - 1) / L;
  uint32_t s = 0;
  while (G > 1) {
    if (s == 16) return false;
    out->arity[s] = 2;
    dkgh::zl_to_bytes(out->mult[s], y);
    y = dkgh::zl_mul(y, y);
    G = (G + 1) / 2;
    s++;
  }
  out->stages = s;
  return true;
}

}  // namespace

extern "C" {

// The fitted rule ("one party's checks"; profiles/receivers_time.json): a launch
// costs RP_LAUNCH_US, a dependent point operation RP_LAT_US while the launch leaves the SIMDs
// under-occupied, and n lanes' worth of operations RP_THR_US each once the device is full.  The serial
// walk is k_horner, built with the product-scanning field multiplication: its dependent operation
// costs RP_SERIAL_LAT_US.  A plan with fold stages also pays RP_SETUP_US on the host side of the call
// (its indices and digits are uploaded).
static const double RP_LAUNCH_US = 7.1, RP_LAT_US = 2.0, RP_THR_US = 2.2e-5, RP_SERIAL_LAT_US = 2.77,
                    RP_SETUP_US = 1.75;

void dkg_receiver_plan_constants(double c[5]) {
  if (!c) return;
  c[0] = RP_LAUNCH_US, c[1] = RP_LAT_US, c[2] = RP_THR_US, c[3] = RP_SERIAL_LAT_US, c[4] = RP_SETUP_US;
}

double dkg_receiver_plan_cost_us(size_t n, size_t t, uint32_t x, const dkg_receiver_plan* p) {
  if (!p || !n || !x) return -1.0;
  const size_t N = t + 1;
  uint8_t xb[32];
  u32_bytes(xb, x);
  const double cx = chain_ops(xb) + 1, lanes = (double)((n + 63) / 64 * 64);
  const size_t L = p->chunk < N ? p->chunk : N;
  size_t G = (N + L - 1) / L;
  const double lat = p->stages ? RP_LAT_US : RP_SERIAL_LAT_US;
  double us = (p->stages ? RP_SETUP_US : 0.0) + RP_LAUNCH_US + lat * (double)(L - 1) * cx + RP_THR_US * lanes * (double)(N - G) * cx;
  for (uint32_t s = 0; s < p->stages; s++) {
    const size_t r = p->arity[s], Gout = (G + r - 1) / r;
    const double cy = chain_ops(p->mult[s]) + 1;
    us += RP_LAUNCH_US + RP_LAT_US * (double)(r - 1) * cy + RP_THR_US * lanes * (double)(G - Gout) * cy;
    G = Gout;
  }
  return us;
}

int dkg_pair_eval_shape(size_t t, int chunk, uint32_t* L, uint32_t* lanes, uint32_t* stages) {
  if (!L || !lanes || !stages || chunk < 0 || t >= 0xffffffffu) return DKG_E_ARG;
  const size_t N = t + 1;
  size_t l = chunk ? (size_t)chunk : (N + 63) / 64;
  if (l > N) l = N;  // one lane walks the whole row
  const size_t g = (N + l - 1) / l;
  if (g > 64) return DKG_E_ARG;
  uint32_t s = 0;
  while (((size_t)1 << s) < g) s++;
  *L = (uint32_t)l, *lanes = (uint32_t)g, *stages = s;
  return DKG_OK;
}

int dkg_receiver_plan_for(size_t n, size_t t, uint32_t x, int chunk, dkg_receiver_plan* out) {
  if (!out || n == 0 || x == 0 || (size_t)x > n || chunk < 0) return DKG_E_ARG;
  const size_t N = t + 1;
  if (chunk > 0) return fill_plan(N, x, (size_t)chunk, out) ? DKG_OK : DKG_E_ARG;
  // automatic: the cheapest of the serial walk and the power-of-two chunks by the fitted rule
  dkg_receiver_plan best;
  fill_plan(N, x, N, &best);
  double best_us = dkg_receiver_plan_cost_us(n, t, x, &best);
  uint8_t xb[32];
  u32_bytes(xb, x);
  const long serial_chain = (long)(N - 1) * (chain_ops(xb) + 1);
  for (size_t L = 2; L < N && L <= 64; L *= 2) {
    dkg_receiver_plan p;
    if (!fill_plan(N, x, L, &p)) continue;
    long chain = (long)(L - 1) * (chain_ops(xb) + 1);
    for (uint32_t k = 0; k < p.stages; k++) chain += (long)(p.arity[k] - 1) * (chain_ops(p.mult[k]) + 1);
    if (chain > serial_chain) continue;  // a longer chain AND more work and launches never pays
    const double us = dkg_receiver_plan_cost_us(n, t, x, &p);
    if (us < best_us) best_us = us, best = p;
  }
  *out = best;
  return DKG_OK;
}

// The seats' rule ("seats of large committees"; profiles/seat_chunks_time.json), in
// the form of dkg_receiver_plan_cost_us with 64 * waves lanes: a launch costs SE_LAUNCH_US, a dependent
// point operation of k_seat_chunks / k_seat_fold SE_LAT_US, one of k_seat_horner SE_SERIAL_LAT_US, a
// lane's operation SE_THR_US once the device is full, and a chunked call SE_SETUP_US for its digit
// records, its scratch and the upload.  The rule's estimates miss the record's device times by up to a
// quarter, so a chunked shape is taken only where its estimate is below SE_MARGIN times the serial one.
static const double SE_LAUNCH_US = 7.1, SE_LAT_US = 1.5, SE_THR_US = 2.6e-5, SE_SERIAL_LAT_US = 1.95,
                    SE_SETUP_US = 25.0, SE_MARGIN = 0.8;
static const uint64_t SE_SCRATCH_MAX = (uint64_t)1 << 30;

void dkg_seat_eval_constants(double c[6]) {
  if (!c) return;
  c[0] = SE_LAUNCH_US, c[1] = SE_LAT_US, c[2] = SE_THR_US, c[3] = SE_SERIAL_LAT_US, c[4] = SE_SETUP_US;
  c[5] = SE_MARGIN;
}

int dkg_seat_eval_shape(size_t n, size_t t, size_t waves, uint32_t x_max, int chunk, uint32_t* L, uint32_t* G,
                        uint32_t* stages, uint64_t* scratch_bytes) {
  if (!L || !G || !stages || !scratch_bytes || n == 0 || waves == 0 || x_max == 0 || (size_t)x_max > n || chunk < 0 ||
      t >= 0xffffffffu || waves > 0xffffffffu)
    return DKG_E_ARG;
  const size_t N = t + 1;
  // Q and its ping-pong partner, [40][G][64 waves] words each; none for the serial walk
  auto scratch = [&](size_t g) { return g > 1 ? (uint64_t)2 * 160 * g * 64 * waves : (uint64_t)0; };
  if (chunk > 0) {
    const size_t l = std::min((size_t)chunk, N), g = (N + l - 1) / l;
    dkg_receiver_plan p;
    // k_seat_chunks runs the chunks along grid.y; 65535 of them fold in 16 stages, so the second test never fires
    if (g > 65535 || !fill_plan(N, x_max, l, &p)) return DKG_E_ARG;
    *L = (uint32_t)l, *G = (uint32_t)g, *stages = p.stages, *scratch_bytes = scratch(g);
    return DKG_OK;
  }
  uint8_t xb[32];
  u32_bytes(xb, x_max);
  const double cx = chain_ops(xb) + 1, lanes = 64.0 * (double)waves;
  const long serial_chain = (long)(N - 1) * (long)cx;
  double best_us = SE_LAUNCH_US + SE_SERIAL_LAT_US * (double)serial_chain + SE_THR_US * lanes * (double)serial_chain;
  size_t best_l = N, best_g = 1;
  uint32_t best_s = 0;
  for (size_t l = 2; l < N && l <= 64; l *= 2) {
    dkg_receiver_plan p;
    size_t g = (N + l - 1) / l;
    if (g > 65535 || scratch(g) > SE_SCRATCH_MAX || !fill_plan(N, x_max, l, &p)) continue;
    long chain = (long)(l - 1) * (long)cx;
    double us = SE_SETUP_US + SE_LAUNCH_US + SE_LAT_US * (double)chain + SE_THR_US * lanes * (double)(N - g) * cx;
    for (uint32_t s = 0; s < p.stages; s++) {
      const double cy = chain_ops(p.mult[s]) + 1;
      const size_t gout = (g + 1) / 2;
      chain += (long)cy;
      us += SE_LAUNCH_US + SE_LAT_US * cy + SE_THR_US * lanes * (double)(g - gout) * cy;
      g = gout;
    }
    if (chain > serial_chain) continue;  // as dkg_receiver_plan_for: a longer chain and more work never pays
    us /= SE_MARGIN;  // best_us is the serial estimate, or a chunked one already divided
    if (us < best_us) best_us = us, best_l = l, best_g = (N + l - 1) / l, best_s = p.stages;
  }
  *L = (uint32_t)best_l, *G = (uint32_t)best_g, *stages = best_s, *scratch_bytes = scratch(best_g);
  return DKG_OK;
}

}  // extern "C"
