// Round 1 of an operator's hosted seats (seat_deal.hip): the joint K = pk * r chain of a dealing seat,
// and its scalar recoding as one routine for the host and the device.  All pointers of the launcher are
// device pointers; the launch goes to `stream`.  One copy only: dkg_ctx_set_field_mode does not apply.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace dkgk {

// Signed radix-4 recoding of a scalar k < 2^255 (eight 32-bit words, little-endian), right to left:
// window w holds bits 2w, 2w + 1 plus the carry of the window below; a value of 2 or more gives up 4 and
// carries 1, so the digits are in {-2, -1, 0, 1}.  The top window (127: bit 254 and the dropped bit 255)
// keeps its value instead -- {0, 1, 2}, and {0, 1} for k < 2^254, every canonical scalar among them --
// as the top radix-16 digit of k_benc_mul does.  sum_w digit_w 4^w = k.
constexpr int SEAT_ENC_WINDOWS = 128;

// The two bits of window win, given word win / 16 of the scalar (the kernel picks the word by selects: its
// words are registers).
constexpr uint32_t seat_enc_bits(uint32_t word, int win) { return (word >> (2 * (win & 15))) & 3u; }

// Window win's digit from its bits and the carry in; leaves the carry out in `carry`.
constexpr int seat_enc_digit(uint32_t bits, int win, int& carry) {
  const int d = (int)bits + carry;
  carry = (win < SEAT_ENC_WINDOWS - 1 && d >= 2) ? 1 : 0;
  return d - (carry << 2);
}

// K[(slot) * 2 + w] = r[slot][w] * pk_ext[kbase[slot / n] + slot % n] for slot < slots (slot = seat p * n
// + recipient q; kbase[p] = the first decoded key of seat p's ceremony).  r [slots][2][8] canonical;
// pk_ext SoA [40][stride]; K_ext SoA [40][count], count >= 2 * slots.
void seat_enc_mul(size_t slots, size_t n, const uint32_t* kbase, const uint32_t* r, const uint32_t* pk_ext,
                  size_t stride, uint32_t* K_ext, size_t count, hipStream_t stream);
// seat-to-slot gather index of the per-slot key copies the radix-16 comb route reads: idx[slot] =
// kbase[slot / n] + slot % n
void seat_key_index(size_t slots, size_t n, const uint32_t* kbase, uint32_t* idx, hipStream_t stream);

}  // namespace dkgk
