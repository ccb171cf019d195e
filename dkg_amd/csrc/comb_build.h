// Host-side launchers of the chained comb builder (comb_build.hip).  All pointers are device
// pointers; all launches go to `stream`.  kind 0 = the shared bases' comb (radix 2^DKG_COMBW_BITS),
// kind 1 = the member keys' comb (radix 2^DKG_KEY_COMB_BITS); layouts as points.h CombGeo.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace dkgk {

// The geometry of a kind (host only): false for a kind that does not exist.  chunk = the entries one
// thread of the chained builder walks and inverts together.
bool comb_geometry(int kind, int* bits, int* windows, uint32_t* entries, uint32_t* chunk);
// words of the window-base scratch the chained builder needs for `count` bases
size_t comb_chain_scratch_words(int kind, size_t count);
// combs of the decoded points ext[.., e0 + c], c < count, into tab + c * WORDS(kind): the tables
// build_combw / build_key_combs (kernels.hip) write, by running additions
void build_comb_chained(int kind, const uint32_t* ext, size_t stride, size_t e0, uint32_t* tab, uint32_t* scratch,
                        hipStream_t stream, size_t count);
// entries first .. first + count - 1 of `window` of one table as canonical bytes: out [count][24] words
// (y+x | y-x | 2dxy, fe_tobytes32 each)
void comb_entries_bytes(int kind, const uint32_t* tab, int window, uint32_t first, uint32_t count, uint32_t* out,
                        hipStream_t stream);

}  // namespace dkgk
