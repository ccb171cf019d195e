// Host-side launchers of the hosted seats' rounds 3 and 5 (seat_finalise.hip).  All pointers are device
// pointers; all launches go to `stream`.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace dkgk {

constexpr uint32_t SEAT_ROW_NONE = 0xffffffffu;
// most points (the seat's own + the disclosures of one dealer) k_seat_lagrange stages in LDS
constexpr size_t SEAT_LAGRANGE_MAX_POINTS = 7680;  // 8 B each: 60 KB

// Phases<Phase2>::proceed per seat (committee.rs:453-467): fs[p] = sum over dealers i with
// qualified[scer[p] * n + i] of s[p][i] (canonical [S][n][8]); one wave per seat, lanes over the dealers.
void seat_share_sum(size_t S, size_t n, const uint32_t* scer, const uint8_t* qualified, const uint32_t* s,
                    uint32_t* fs, hipStream_t stream);
// Phases<Phase5>::finalise's interpolations per seat (committee.rs:745-789), one 64-lane workgroup per
// seat: sigma[p] = sum over the reconstructed dealers of seat p's ceremony of the interpolation at zero
// through the seat's own point (sx[p], s[p][dealer]) and the disclosures listed for that dealer, the
// one by sender sx[p] skipped.  Ceremony slot sslot[p] owns the dealer records rptr[slot] ..
// rptr[slot + 1]; record k is dealer rdeal[k] with the disclosures dptr[k] .. dptr[k + 1] of dx (the
// senders' 1-based indices, distinct within a record, < 2^24) and dy [..][8] (canonical shares).
// skip[p] != 0: sigma[p] = 0 without any work.  max_points >= every record's length + 1, at most
// SEAT_LAGRANGE_MAX_POINTS (nothing is launched otherwise).
void seat_lagrange(size_t S, size_t n, const uint32_t* sslot, const uint32_t* sx, const uint8_t* skip,
                   const uint32_t* rptr, const uint32_t* rdeal, const uint32_t* dptr, const uint32_t* dx,
                   const uint32_t* dy, const uint32_t* s, size_t max_points, uint32_t* sigma, hipStream_t stream);
// dst[p] = src[idx[p]] (extended points, word strides sstride / dstride), p < count; idx[p] ==
// SEAT_ROW_NONE leaves dst[p] as it is
void seat_gather_points(size_t count, const uint32_t* idx, const uint32_t* src, size_t sstride, uint32_t* dst,
                        size_t dstride, hipStream_t stream);

}  // namespace dkgk
