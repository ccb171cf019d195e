// Host-side helpers of the product library (not the oracle): BLAKE2b-512 for the commitment key
// (commitment.rs:13-17), the ChaCha20Rng stream for seeded synthetic coefficients, and small
// Z_l arithmetic for the (cold) reconstruction path of finalise (polynomial.rs:162-184).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "seat_map.h"

namespace dkgh {

void blake2b(uint8_t* out, size_t outlen, const uint8_t* in, size_t inlen);
// ChaCha20 keystream (key = seed, 64-bit block counter from `block`, zero stream id)
void chacha20(const uint8_t key[32], uint64_t block, uint8_t* out, size_t len);
// RFC 8439 ChaCha20 (96-bit nonce, 32-bit counter from 0) XOR -- chacha20 0.7 `ChaCha20`, used by
// SymmetricKey::process (elgamal.rs:172-193) on the (cold) complaint-proof path
void chacha20_ietf_xor(uint8_t* out, const uint8_t* in, size_t len, const uint8_t key[32], const uint8_t nonce[12]);

struct Zl {  // canonical element of Z_l, little-endian 64-bit limbs
  uint64_t w[4];
};
Zl zl_from_bytes_wide(const uint8_t* in, size_t len);  // any length, big-endian fold of LE bytes
Zl zl_from_bits(const uint8_t in[32]);  // Scalar::from_bits (groups.rs:29-36): bit 255 dropped, reduced
Zl zl_from_u64(uint64_t x);
void zl_to_bytes(uint8_t out[32], const Zl& a);
Zl zl_add(const Zl& a, const Zl& b);
Zl zl_sub(const Zl& a, const Zl& b);
Zl zl_mul(const Zl& a, const Zl& b);
Zl zl_inv(const Zl& a);
bool zl_is_zero(const Zl& a);

// lattice.cpp: a short (b, a_1, .., a_{K-1}) with a_u = b y^u (mod l), b > 0, 2 <= K <= 5, as
// magnitudes (32 bytes LE) and signs; (1, y, .., y^(K-1)) when no shorter row checks out.
// jsf: price the candidate rows for the pairwise joint-sparse-form chain instead of per-scalar NAFs.
bool short_multipliers(const Zl& y, int K, uint8_t (*mag)[32], int8_t* sign, bool jsf = false);
// Joint sparse form of two 256-bit magnitudes (lattice.cpp); false if it does not fit 256 positions.
bool jsf_digits(const uint8_t a[32], const uint8_t b[32], int8_t* da, int8_t* db, int16_t* top,
                int npos = 256);

// receiver_plan.cpp: the NAF of a little-endian 256-bit value as +1 / -1 digit bits; returns its
// length (the top digit is +1 at length - 1; 0 for zero), *weight (may be null) its nonzero digits.
int naf256(const uint8_t v[32], uint32_t pos[8], uint32_t neg[8], int* weight);
// receiver_plan.cpp: the distinct values of v [count] in order of first appearance and place[p] = where
// v[p] stands among them (the pair evaluation's distinct rows and distinct indices)
void distinct_places(size_t count, const uint32_t* v, std::vector<uint32_t>& distinct, std::vector<uint32_t>& place);

// seat_pack.cpp: what one seats call uploads for k_seat_horner, from dkg_seat_pack's placement.  Wave v
// evaluates at x = wave_desc[2v] the dealers wave_desc[2v + 1] * 64 + i, i < width, of the seats
// wave_seat[v * per_wave + slot] (SEAT_NONE: an empty slot); seat p's commitments are ceremony slot
// seat_col[p] among the distinct ceremonies `cers` (order of first appearance), the only ones decoded.
using ::SEAT_NONE;  // seat_map.h
struct SeatPlan {
  uint32_t width = 0, per_wave = 0, tiles = 0, waves = 0;
  std::vector<uint32_t> cers, seat_col, seat_x, wave_desc, wave_seat;
  size_t live_lanes = 0;  // S n of the 64 waves lanes
};
// DKG_E_ARG for cer[p] >= B, 2^32 - 1 seats or more, and whatever dkg_seat_pack rejects
int seat_plan(size_t B, size_t n, size_t S, const uint32_t* cer, const uint32_t* js, SeatPlan& out);

}  // namespace dkgh
