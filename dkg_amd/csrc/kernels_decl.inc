// Declarations of the kernels.hip launchers, in namespace `dkgk` -- or, included with `dkgk`
// defined as a macro (kernels_ilp.h, and kernels.hip compiled with DKG_FE_ILP), in the namespace
// of the second copy of the kernels built with the column-sum field multiplication.  No include
// guard on purpose: kernels.h and kernels_ilp.h include it once each.
namespace dkgk {

// K5: 32-byte encodings [count][8 words] -> extended SoA [40][stride]; ok[e] = 1 if valid.
void decode_points(const uint32_t* comp, size_t count, uint32_t* ext, size_t stride, uint8_t* ok,
                   hipStream_t stream);
// K5 straight into the binomial's position-major layout: D dealers x N commitments ([D][N][8],
// dealer-major) -> [40][N][npad].  nseg segments are interleaved in 64-column groups: dealer i of
// segment seg lands in column (i / 64) * 64 * nseg + seg * 64 + i % 64; ok[column * N + k].
// k_decode's placement for points already in extended form (src [D][N], word stride sstride)
void place_position_major(const uint32_t* src, size_t sstride, size_t D, size_t N, size_t npad, uint32_t* out,
                          hipStream_t stream, int nseg = 1, int seg = 0, size_t L = 0, size_t pstride = 0);
// dst[i] = src[i * step + k0], i < count (extended points)
void gather_points(const uint32_t* src, size_t sstride, size_t step, size_t k0, size_t count, uint32_t* dst,
                   size_t dstride, hipStream_t stream);
// npad = the table's row width (columns); with a degree split (L < N) coefficient k of column c goes
// to position k % L, column (k / L) * pstride + c, in a table of L rows.
void decode_position_major(const uint32_t* comp, size_t D, size_t N, size_t npad, uint32_t* out, uint8_t* ok,
                           hipStream_t stream, int nseg = 1, int seg = 0, size_t L = 0, size_t pstride = 0);
// every column of a position-major table [40][S] set to the identity
void fill_identity(size_t S, uint32_t* out, hipStream_t stream);
// fused round-2/4 check over interleaved E/A columns (see k_check_both): dealers
// [dealer0, dealer0 + ndealers) of this call, s / sp / dec2 / dec4 indexed dealer * nrecv + j from
// their bases, self = (dealer + dealer_base) mod nmod == j.
// scale (may be null): [nrecv][8] words, b_j 2^256 mod l: R holds b_j P(j) (combine_short) and the
// shares are taken to b_j s before the fixed-base products.
// acc (may be null: one fused launch): [ndealers * jn][40] words; the g and h combs then run as two
// launches with g*s parked in acc (each launch reads one 3.1-MB comb).
void check_both(size_t ndealers, size_t nrecv, size_t dealer0, size_t dealer_base, size_t nmod, const uint32_t* s,
                const uint32_t* sp, const uint32_t* R, const uint32_t* tab_g, const uint32_t* tab_h,
                const uint8_t* dok, uint8_t* dec2, uint8_t* dec4, hipStream_t stream, const uint32_t* scale = nullptr,
                size_t j0 = 0, size_t jn = 0, uint32_t* acc = nullptr);
// extended SoA -> encodings [count][8]
void encode_points(const uint32_t* ext, size_t stride, size_t count, uint32_t* comp, hipStream_t stream);
// comb tables of the decoded points ext[.., e0 + c], c < count, into tab + c * 15360 (30 x 512 words each)
void build_comb(const uint32_t* ext, size_t stride, size_t e0, uint32_t* tab, hipStream_t stream, size_t count = 1);
// radix-2^10 combs (COMBW_WORDS words each) of `count` points: the tables of commit / check /
// fixed_base (global memory, L2-resident)
void build_combw(const uint32_t* ext, size_t stride, size_t e0, uint32_t* tab, hipStream_t stream, size_t count = 1);

// K2: A_k = g a_k, E_k = A_k + h b_k for D*N coefficients (scalars [D*N][8]); outputs SoA [40][DN].
// The commitments of dealers [0, D) (coefficients a, b [D][N][8]) straight into a fused (E, A)
// position-major table: out = the table at the dealers' first column group, W its column count,
// L the piece length, pstride the piece stride; A0 [40][A0stride] receives A_i0 (element i).
void commit_position_major(size_t D, size_t N, const uint32_t* a, const uint32_t* b, const uint32_t* tab_g,
                           const uint32_t* tab_h, uint32_t* out, size_t W, size_t L, size_t pstride, uint32_t* A0,
                           size_t A0stride, hipStream_t stream);
// stride (0: count): word stride of the A_ext / E_ext planes (a slice of a larger SoA array)
void commit(size_t count, const uint32_t* a, const uint32_t* b, const uint32_t* tab_g,
            const uint32_t* tab_h, uint32_t* A_ext, uint32_t* E_ext, hipStream_t stream, size_t stride = 0);
// K1: s[i][j] = f_i(j+1), s'[i][j] = f'_i(j+1) (scalars [D][n][8]); coefficients [D][N][8].
void share_eval(size_t D, size_t n, size_t N, const uint32_t* a, const uint32_t* b, uint32_t* s,
                uint32_t* sp, hipStream_t stream);
// Polynomial::evaluate for D polynomials at M small integer points x[m] (< 2^24).
void poly_eval(size_t D, size_t N, const uint32_t* coeffs, size_t M, const uint32_t* xs, uint32_t* out,
               hipStream_t stream);

// K3a: binomial-basis Horner.  C: decoded commitments SoA [40][N][npad] (position-major,
// dealer-minor); e0/e1 ping-pong buffers of the same shape.  Processes `width` (multiple of 64)
// dealer columns starting at the given pointers (a dealer chunk: pass C + c0, e0 + c0, e1 + c0).
// Returns the buffer holding e_m = Delta^m P_i(0), m = 0..t.
// pieces > 1: the same for the columns [u * pstride, u * pstride + width) of every piece u
// last_len (0: N): the last piece's length when it is shorter (its coefficients >= last_len are the
// identity); its positions >= last_len are then left unwritten (never read by the stepping).
uint32_t* binomial(size_t width, size_t npad, size_t N, const uint32_t* C, uint32_t* e0, uint32_t* e1,
                   hipStream_t stream, size_t pieces = 1, size_t pstride = 0, size_t last_len = 0);
// binomial() as its two parts: the copy of C_t into position 0 of e0, and Horner step r (1..N-1)
// from table `in` to table `out` (the caller ping-pongs them)
void binom_init(size_t width, size_t npad, size_t N, const uint32_t* C, uint32_t* e0, hipStream_t stream,
                size_t pieces = 1, size_t pstride = 0);
void binom_step(size_t r, size_t width, size_t npad, size_t N, const uint32_t* C, const uint32_t* in, uint32_t* out,
                hipStream_t stream, size_t pieces = 1, size_t pstride = 0, size_t last_len = 0,
                uint32_t* flags = nullptr, size_t col_base = 0, size_t dreal = 0, unsigned gw = 64,
                bool flag_any = false,   // flag_any: flags is one word, set when any group was marked
                bool nt = false,         // nt: nontemporal stores of the step's rows
                bool il = false);        // il: paired products in the m-chain at <= 2 waves per SIMD
// The complete redo of the binomial tables of the (piece, 64-column) groups marked in flags by a
// dedicated pass (binom_step / binomial_wave with flags): per-wave loops from the coefficients into
// e, in place; unmarked groups exit at once.
void binomial_wave_redo(size_t width, size_t npad, size_t N, const uint32_t* C, uint32_t* e, hipStream_t stream,
                        size_t pieces, size_t pstride, size_t last_len, uint32_t* flags, size_t col_base,
                        size_t dreal, unsigned gw);
// binomial() as ONE launch in which each wave runs every step of its 64 columns in place
// (k_binom_wave; tables of many column groups): the table is e itself, which is returned.  eT (may
// be null): the last step writes there instead, column-major as to_column_major(.., eT, ..) would
// (then e holds the table after step N-2 only).  prefetch: each item's operand loaded during the
// previous item's chain (2 waves per SIMD instead of 3).  flags (may be null: complete additions
// throughout): one zeroed word per (piece, 64-column group) of the whole table -- the dedicated
// additions run first and a second launch redoes the groups whose real columns (dealer index below
// dreal; gw columns per dealer group, col_base = this call's first column) met Z = 0.
uint32_t* binomial_wave(size_t width, size_t npad, size_t N, const uint32_t* C, uint32_t* e, hipStream_t stream,
                        size_t pieces = 1, size_t pstride = 0, size_t last_len = 0, uint32_t* eT = nullptr,
                        bool prefetch = false, uint32_t* flags = nullptr, size_t col_base = 0, size_t dreal = 0,
                        unsigned gw = 64);
// binom_step with lane pairs (k_binom_pair, split.h): each column's point on two lanes that share
// its field products; for latency-bound steps.  Identical tables.
void binom_step_pair(size_t r, size_t width, size_t npad, size_t N, const uint32_t* C, const uint32_t* in,
                     uint32_t* out, hipStream_t stream, size_t pieces = 1, size_t pstride = 0, size_t last_len = 0);
// Position-major [40][N][npad] -> column-major [40][npad][N] (element c * N + m) for the columns
// [u * pstride, u * pstride + width) of each of `pieces` pieces (the stepping's input layout).
void to_column_major(size_t width, size_t npad, size_t N, const uint32_t* e, uint32_t* eT, size_t pieces,
                     size_t pstride, hipStream_t stream);
// K3b: finite-difference stepping: R[i][j] = P_i(j+1) for j in [0, nrecv), point-major (AoS)
// [i*nrecv + j][40] (pt_store_aos), from the column-major difference table e (to_column_major;
// word stride N * npad).  stream_a / stream_b: scratch for the inter-block boundary streams, each
// >= ndealers*nrecv*160 B (unused when N <= 512).
// How k_stepping covers an N-position table: nblk blocks of P positions on bs lanes (nblk > 1), or
// `per` tables of P = N lanes each per bs-lane workgroup; maxbs = the LDS variant (192, 256 or 512).
struct StepShape {
  size_t nblk, P, per, bs, maxbs;
};
StepShape stepping_shape(size_t N);
// relative issue rate of a bs-lane workgroup in the maxbs LDS variant (resident waves per SIMD)
double step_occupancy(size_t bs, size_t maxbs);
// true when every piece of a split column fits one workgroup slot ((pieces-1) L + last_len <= 512):
// the stepping then runs one slot per column over all pieces
bool stepping_whole_columns(size_t L, size_t pieces, size_t last_len);
// cost model of stepping()'s launches over `cols` columns: SIMD cycles per (receiver step x
// instruction of one addition); compare modes / splits with it.  nrecv > 0: issue-bound rounds pay
// only for the wave-steps whose wave still adds (dead positions: banded or contiguous lane map,
// step_map.h); 0 prices every wave for the whole launch
double stepping_cycles(size_t cols, size_t N, size_t pieces, size_t last_len, bool whole, size_t nrecv = 0);
// resident waves per SIMD in a round of stepping()'s main launch over `cols` columns
double stepping_waves_per_simd(size_t cols, size_t N, size_t pieces, size_t last_len, bool whole);
// last_len (0: N): length of a shorter last piece (its table positions >= last_len are not read)
// whole: run the pieces of a column in one slot when they fit (stepping_whole_columns)
// flags (may be null: complete formula only): stepping_flag_words(ndealers, pieces) zeroed words;
// the additions then run by the dedicated formula and the workgroups that met an exceptional pair
// are redone with the complete one (kernels.hip k_stepping).
size_t stepping_flag_words(size_t ndealers, size_t pieces);
// test aid (dkg_zero_tests): out[count][3] = fe_maybe_zero, fe_tight_zero, fe_zero_guard of limbs[count][10]
void zero_tests(size_t count, const uint32_t* limbs, uint8_t* out, hipStream_t stream);
// test aid (dkg_fe_ops): one fe25519.h primitive per lane, in this copy's flavour of the products.  in
// [count][win] and out [count][wout] raw 32-bit words (fe_ops_shape; false for an unknown op): ten limbs
// per element, operands in the primitive's argument order.  MUL2 (fa, ga, fb, gb) and SQ2 (fa, fb) return
// both results; MUL_SMALL takes the limbs and k; TOBYTES returns the 8 words, fe_isneg, fe_iszero;
// FROMBYTES takes 8 words.
enum {
  FE_OP_MUL, FE_OP_SQ, FE_OP_MUL2, FE_OP_SQ2, FE_OP_MUL_SMALL, FE_OP_CARRY, FE_OP_ADD, FE_OP_SUB, FE_OP_NEG,
  FE_OP_DBL, FE_OP_INVERT, FE_OP_POW22523, FE_OP_TOBYTES, FE_OP_FROMBYTES, FE_OP_ABS, FE_OP_COUNT
};
bool fe_ops_shape(int op, size_t* win, size_t* wout);
void fe_ops(int op, size_t count, const uint32_t* in, uint32_t* out, hipStream_t stream);
// test aid (dkg_sc_ops; the product-scanning copy only): one sc25519.h primitive per lane on 32-bit
// words.  REDUCE9 / REDUCE256 / REDUCE512 take 9 / 8 / 16 words; MUL_SMALL_ADD (a, x, c); HORNER2 (a, x,
// c1, c0); LAZY takes (state [10], steps <= SC_LAZY_STEPS, x, coefficient [8]), runs the steps and
// sc_lazy_fold, and returns the folded state [10] and sc_lazy_final [8]; RADIX16 returns the 64 signed
// digits as bytes, four to a word.
enum {
  SC_OP_REDUCE9, SC_OP_REDUCE256, SC_OP_REDUCE512, SC_OP_ADD, SC_OP_SUB, SC_OP_NEG, SC_OP_MUL_SMALL_ADD,
  SC_OP_HORNER2, SC_OP_LAZY, SC_OP_MONT_MUL, SC_OP_MUL, SC_OP_MONT_INV, SC_OP_RADIX16, SC_OP_COUNT
};
bool sc_ops_shape(int op, size_t* win, size_t* wout);
uint32_t sc_ops_lazy_steps();  // SC_LAZY_STEPS of sc25519.h
void sc_ops(int op, size_t count, const uint32_t* in, uint32_t* out, hipStream_t stream);
// Rz (may be null): also a dense copy of every stored point's Z, 10 words per point at the index of
// R (read by affine_pieces).
// col0, dreal, gw: column c (0-based within this call) is global table column col0 + c of dealer
// groups of gw columns (64 per segment); only columns of dealers < dreal mark their workgroup
// (identity padding columns always meet Z = 0 in the dedicated formula).
// tail_a, tail_b (may be null): scratch for the dead-position repack (stepping_tail_phases > 1,
// one unsplit table), laid out for the whole table of npad columns (this call's start at col0):
// each >= stepping_tail_words(npad, N) words.
// r_scaled (pieces > 1 only): R and Rz take scaled records (X, Y, 2Z, T/2) (points.h, scaled state:
// the dedicated loop then has no doubling); their one reader must be affine_pairs or affine_pieces
// called with scaled = true, which fold the constants into the normalisation.
// Returns false, with nothing launched past that point, when the launches would need more flag
// words than stepping_flag_words(ndealers, pieces).
bool stepping(size_t ndealers, size_t npad, size_t N, const uint32_t* e, size_t nrecv, uint32_t* R,
              uint32_t* stream_a, uint32_t* stream_b, hipStream_t stream, size_t pieces = 1, size_t pstride = 0,
              size_t last_len = 0, bool whole = true, uint32_t* flags = nullptr, size_t col0 = 0,
              size_t dreal = (size_t)-1, unsigned gw = 64, uint32_t* Rz = nullptr, uint32_t* tail_a = nullptr,
              uint32_t* tail_b = nullptr, bool r_scaled = false);
// Dead-position repack of an unsplit table (DESIGN.md section 4): position p is dead once p + j >=
// nrecv, so from step nrecv - P/2 + 1 on only P/2 positions of a P-lane segment still add.  Phase k
// runs steps [J_k, J_{k+1}) on segments of P_k = N / 2^k lanes (J_k = nrecv - P_k + 1: its top
// lane never adds again), carrying the P_{k+1} live positions to the next phase.  Number of phases
// stepping() runs for (N, nrecv, pieces) (1: no repack), and the words of one scratch state.
int stepping_tail_phases(size_t N, size_t nrecv, size_t pieces);
size_t stepping_tail_words(size_t ndealers, size_t N);
// Degree-split recombination: R[c][j] = sum_u y_j^u R[u * pstride + c][j] (pairwise Horner in y^2
// with joint NAF chains; digits [n][2][256] = NAF of y_j and y_j^2, top [n][2])
void combine(size_t width, size_t pstride, size_t pieces, size_t nrecv, const int8_t* digits, const int16_t* top,
             uint32_t* R, hipStream_t stream);
// The same with short multipliers (2 <= pieces <= 4): R[c][j] = sum_u v_ju R[u * pstride + c][j] =
// b_j P(j) for the short lattice vector v_j = (b_j, ..) of runtime.hip split_short (digits [n][256]
// words, byte u = the signed NAF digit of v_ju; top [n])
void combine_short(size_t width, size_t pstride, size_t pieces, size_t nrecv, const uint32_t* digits,
                   const int16_t* top, uint32_t* R, hipStream_t stream);
// Affine addends for combine_short: A[(u * pstride + c) * nrecv + j] (32-word slots: y+x, y-x, 2dxy,
// 2 pad) = the affine Niels form of R's piece value at the same index, for every piece u < pieces
// and column c < width (Montgomery's trick over runs of receivers, one inversion per run).
// j0, jn (0: the rest): receivers [j0, j0 + jn) only.  scaled: R and Rz hold stepping()'s r_scaled records.
void affine_pieces(size_t width, size_t pstride, size_t pieces, size_t nrecv, const uint32_t* R, uint32_t* A,
                   hipStream_t stream, const uint32_t* Rz = nullptr, size_t j0 = 0, size_t jn = 0,
                   bool scaled = false);
// combine_short reading its addends from affine_pieces' A (mixed additions, 7M instead of 8M); the
// result b_j P(j) goes to R[c][j] as in combine_short.
void combine_short_aff(size_t width, size_t pstride, size_t pieces, size_t nrecv, const uint32_t* digits,
                       const int16_t* top, const uint32_t* A, uint32_t* R, hipStream_t stream, size_t j0 = 0,
                       size_t jn = 0);
// Pairwise joint sparse form (pieces = 2 or 4).  affine_pairs is affine_pieces for the JSF chains: it
// writes the affine addends of the pieces AND of Q_2p + Q_2p+1 and Q_2p - Q_2p+1 of every pair p, the
// latter as planes pieces + 2p and pieces + 2p + 1 of A, so A holds pieces + 2 floor(pieces / 2)
// planes of pstride columns and R only the pieces' (the projective sums are never stored; one
// inverse serves a pair's sum and difference).  It reads Z from R itself: no dense Z copy.
// scaled: R holds stepping()'s r_scaled records.
void affine_pairs(size_t width, size_t pstride, size_t pieces, size_t nrecv, const uint32_t* R, uint32_t* A,
                  hipStream_t stream, size_t j0 = 0, size_t jn = 0, bool scaled = false);
// combine_short_aff over JSF digits (runtime.hip split_short): a column with both digits of a pair
// set adds the pair's sum or difference, streamed from its plane of A one such column ahead.
// ev [nrecv][JSF_EV_WORDS]: one word per both-nonzero column in chain order -- positions downwards,
// pair 0 before pair 1: bits 0-1 the plane after the pieces' (2 pair + 1 if the digits differ), bit
// 2 set if the pair's first digit is negative -- then JSF_EV_NONE to the end of the row.
constexpr uint32_t JSF_EV_NONE = 0xffu;
constexpr size_t JSF_EV_WORDS = 384;  // <= 2/3 of 256 positions per pair, two pairs, two ahead
void combine_short_jsf(size_t width, size_t pstride, size_t pieces, size_t nrecv, const uint32_t* digits,
                       const int16_t* top, const uint32_t* ev, const uint32_t* A, uint32_t* R, hipStream_t stream,
                       size_t j0 = 0, size_t jn = 0);
// K3c: decision[i][j] = (g s_ij + h s'_ij == R[i][j]) (round 2) or (g s_ij == R[i][j]) (round 4);
// dealer_ok[i] == 0 forces 0; self ((i + dealer_base) mod nmod == j + recv_base, nmod = parties per
// ceremony, so batched ceremonies stacked dealer-wise work too) gives 2.
// R: point-major (AoS) [i*nrecv + j][40].
void check(size_t ndealers, size_t nrecv, size_t dealer_base, size_t recv_base, size_t nmod, int round,
           const uint32_t* s, const uint32_t* sp, const uint32_t* R, const uint32_t* tab_g,
           const uint32_t* tab_h, const uint8_t* dealer_ok, uint8_t* decision, hipStream_t stream,
           const uint32_t* scale = nullptr);
// dok[column of dealer i of segment seg] &= extra[i] (verify_device's interleaved column layout)
void and_dealer_mask(size_t D, int nseg, int seg, const uint8_t* extra, uint8_t* dok, hipStream_t stream);
// per-dealer validity: dealer_ok[i] = AND of point_ok over its N commitments (dealer-major [D][N])
void dealer_ok(size_t ndealers, size_t N, const uint8_t* point_ok, uint8_t* ok, hipStream_t stream);
// Horner in the exponent for receivers x0 .. x0+nrecv-1 (1-based indices): R point-major [ndealers*nrecv][40]
void horner(size_t ndealers, size_t npad, size_t N, const uint32_t* C, uint32_t x0, size_t nrecv, uint32_t* R,
            hipStream_t stream);
// out column col + g (SoA, stride ostride) = sum over e in [g*count, (g+1)*count) of mask[e] * P_e
// (mask may be NULL), for each group g < groups.
void sum_points(size_t count, const uint32_t* pts, size_t stride, const uint8_t* mask, uint32_t* out, size_t ostride,
                size_t col, hipStream_t stream, size_t groups = 1);
// out[e] = a[e] + b[e] for SoA point vectors of the same stride (out may alias a)
void add_points(size_t count, const uint32_t* a, const uint32_t* b, size_t stride, uint32_t* out, hipStream_t stream);
// Decision-matrix summaries for `groups` stacked ceremonies of n parties (dec [groups*n][n]):
// row_reject[i] = any REJECT in row i; complaints[g][j] = REJECTs by receiver j in group g.
// out[g*n+j] = 1 + #{qualified i : dec[g][i][j] == ACCEPT} < t + 1 (round-4 MisbehaviourHigherThreshold)
void r4_error(size_t groups, size_t n, size_t t, const uint8_t* dec, const uint8_t* qmask, uint8_t* out,
              hipStream_t stream);
void decision_summary(size_t groups, size_t n, const uint8_t* dec, uint8_t* row_reject, int32_t* complaints,
                      hipStream_t stream);
// dec[g*n+i][j] = SKIPPED for j != i when qmask[g*n+i] == 0 (committee.rs:522)
void apply_skipped(size_t groups, size_t n, uint8_t* dec, const uint8_t* qmask, hipStream_t stream);
// out [n][width] = the valid rows of the all-gathered per-rank blocks in [ws][R][width] (rank r holds
// dealers [r*n/ws, (r+1)*n/ws)); any width and alignment (vectorised when both allow)
void compact_ranks(size_t n, size_t ws, size_t R, size_t width, const void* in, void* out, hipStream_t stream);
// out[i] = !a[i] && (b == NULL || b[i]) over V bytes
void mask_not_and(size_t V, const uint8_t* a, const uint8_t* b, uint8_t* out, hipStream_t stream);
// out[i] = row i of dec [rows][n] holds a REJECT or MISSING (k_row_reject)
void row_reject(size_t rows, size_t n, const uint8_t* dec, uint8_t* out, hipStream_t stream);
// the member keys' global combs (radix 2^DKG_KEY_COMB_BITS): words per key and the builder
size_t key_comb_words();
int key_comb_windows();
void build_key_combs(const uint32_t* ext, size_t stride, size_t e0, uint32_t* tab, hipStream_t stream,
                     size_t count);
// windows (mixed additions) per scalar of the radix-2^DKG_COMBW_BITS fixed-base combs
int fixed_base_windows();
// packed decision rows (kernels.hip k_pack_rows): [rows][ceil(n/32) + 1] words from [rows][n] bytes of
// dealers d0.. (rows >= nvalid zero); err[0] set when a row does not fit the encoding
void pack_rows(size_t rows, size_t nvalid, size_t n, size_t d0, const uint8_t* dec, uint32_t* out, uint32_t* err,
               hipStream_t stream);
// all-gathered packed blocks [ws][R][ceil(n/32) + 1] -> dense [n][n] decision bytes
void unpack_ranks(size_t n, size_t ws, size_t R, const uint32_t* in, uint8_t* out, hipStream_t stream);
// hash_to_group tail: from_uniform_bytes(64 bytes as 16 LE words) -> SoA point (stride 1)
void from_uniform(const uint32_t* in16, uint32_t* out, hipStream_t stream);

// Generic batched MSM (trait boundary): out[b] = sum_k scalars[b][k] * points[b][k];
// points given decoded SoA [40][B*N] (element b*N + k), scalars [B*N][8].
void msm_batch(size_t B, size_t N, const uint32_t* scalars, const uint32_t* pts, size_t stride, uint32_t* tab,
               uint32_t* out_ext, hipStream_t stream);
// Fixed-base batch: out = s * base via comb table; out SoA [40][count]
void fixed_base(size_t count, const uint32_t* scalars, const uint32_t* tab, uint32_t* out_ext,
                hipStream_t stream);
// Transpose dealer-major point SoA [40][D*N] (element i*N+k) to position-major [40][N][npad].
void to_position_major(size_t D, size_t N, size_t npad, const uint32_t* in, uint32_t* out,
                       hipStream_t stream);
// Scalar reduction of 256-bit inputs to canonical (from_bits semantics, groups.rs:29-36: bit 255 dropped).
void reduce_scalars(size_t count, const uint32_t* in, uint32_t* out, hipStream_t stream);
// Modular sum over dealers with mask: out[j] = sum_i mask[i] * s[i][j]  (round-3 final share)
void sum_shares(size_t D, size_t n, const uint32_t* s, const uint8_t* mask, uint32_t* out, hipStream_t stream,
                size_t groups = 1);
// On-device synthetic coefficients (seedgen.hip): rows r in [0, rows) are dealer d0 + r % D of
// ceremony c0 + r / D; a, b [rows][N][8] canonical, identical to the host dkg_dealer_coeffs.
// master: 8 words on the device; seeds: scratch [rows][8].
void dealer_coeffs(size_t rows, size_t D, size_t d0, uint32_t c0, const uint32_t* master, size_t N, uint32_t* seeds,
                   uint32_t* a, uint32_t* b, hipStream_t stream);

// ---- full (encrypted-share) mode, hybrid.hip (elgamal.rs:134-193) ----
// Items are (dealer i, recipient q, w) at index (i * n + q) * 2 + w; w = 0 is the randomness (s')
// ciphertext, w = 1 the share (s) ciphertext (committee.rs:171-172 order).
// R = g r, K = pk_q r for every item (r [items][8]); tab_gw: the generator's radix-2^10 comb;
// tabs_pk: one (radix-16) comb table per recipient.
void enc_mul(size_t D, size_t n, const uint32_t* r, const uint32_t* tab_gw, const uint32_t* tabs_pk, uint32_t* R_ext,
             uint32_t* K_ext, hipStream_t stream);
// K = sk_q * R for every item, R decoded SoA [40][items] (sk [n][8], wave-uniform per recipient)
void dec_mul(size_t D, size_t n, const uint32_t* sk, const uint32_t* R_ext, uint32_t* K_ext, hipStream_t stream,
             uint32_t* table = nullptr);
// words of dec_mul's odd-multiples table (the width-4 window; 0 when built with -DDKG_DEC_NAF)
size_t dec_mul_table_words(size_t D, size_t n);
// SymmetricKey::process: keystream from Blake2b-512(Kc) (Kc [items][8] encodings).
// encrypt: ct[item] = (w ? s : sp)[i*n+q] ^ ks.  decrypt: (w ? s : sp)[i*n+q] = reduce(from_bits(ct[item] ^ ks)).
void sym_xor(size_t D, size_t n, const uint32_t* Kc, bool decrypt, uint32_t* ct, uint32_t* s, uint32_t* sp,
             hipStream_t stream);
// per-row dealer seeds [rows][8] (row r = dealer d0 + r % D of ceremony c0 + r / D; seedgen.hip)
void dealer_seeds(size_t rows, size_t D, size_t d0, uint32_t c0, const uint32_t* master, uint32_t* seeds,
                  hipStream_t stream);
// encryption randomness rows (seedgen.hip): r [rows][n][2][8] = wide(block 2N + 2q + w) of each dealer stream
void enc_randomness(size_t rows, size_t n, size_t N, const uint32_t* seeds, uint32_t* r, hipStream_t stream);

// ---- full mode for batches of ceremonies, hybrid_batch.hip: key c*n + q belongs to recipient q of
// ceremony c, item (c, i, q, w) sits at ((c*n + i)*n + q)*2 + w
// signed radix-16 combs (benc_tab_words() words each: 64 windows x 8 multiples, cached form) of the
// decoded keys pk_ext[.., key], key < keys
size_t benc_tab_words();
void benc_tab(size_t keys, const uint32_t* pk_ext, size_t stride, uint32_t* tab, hipStream_t stream);
// K = pk_key * r for every item of the keys' ceremonies (r [items][8] canonical), K_ext SoA [40][count];
// rows dealers per key set of n keys (a batch: n; one ceremony's dealer shard: D), item (c, i, q, w) at
// ((c*rows + i)*n + q)*2 + w
void benc_mul(size_t keys, size_t n, size_t rows, const uint32_t* r, const uint32_t* tab, uint32_t* K_ext,
              size_t count, hipStream_t stream);
// K = sk_key * R for every item (sk [keys][8], wave-uniform; R decoded SoA [40][count]); table:
// bdec_mul_table_words(keys, n) words for the width-4 window's odd multiples
size_t bdec_mul_table_words(size_t keys, size_t n);
size_t bdec_launch_waves();  // waves per launch (the table's slots): larger calls run as slices
void bdec_mul(size_t keys, size_t n, const uint32_t* sk, const uint32_t* R_ext, uint32_t* K_ext, size_t count,
              uint32_t* table, hipStream_t stream);
// the same for `seats` keys with n items pairs each and no recipient axis: K = sk_p * R for the items
// (p * n + i) * 2 + w; table: bdec_mul_table_words(seats, n) words
void seat_dec_mul(size_t seats, size_t n, const uint32_t* sk, const uint32_t* R_ext, uint32_t* K_ext, size_t count,
                  uint32_t* table, hipStream_t stream);

// ---- round-2 complaints, complaints.hip (broadcast.rs:50-99, 189-283)
// out[k] = sa[k] P (joint = false, width-2 windows) or sa[k] P + sb[k] Q (Straus), P / Q = elements
// bp[k] / bq[k] of the decoded SoA Pext; scalars canonical [cnt][8]; out SoA [40][cnt];
// T: cmp_ladder_table_words(cnt) words of scratch
size_t cmp_ladder_table_words(size_t cnt);
void cmp_ladder(size_t cnt, bool joint, const uint32_t* bp, const uint32_t* bq, const uint32_t* sa, const uint32_t* sb,
                const uint32_t* Pext, size_t pstride, uint32_t* T, uint32_t* out, hipStream_t stream);
// Three per-complaint index arrays, all 1-based, which one ceremony fills with (accuser, accuser,
// accused) and a batch of stacked ceremonies with different values: the EVALUATION INDEX xs /
// accuser (the accuser within its ceremony: Horner's multiplier, the scale slot), the PARTY ROW
// party (the accuser's slot in pk: g n + accuser) and the COMMITMENT ROW crow (the accused's row of
// the decoded commitments, of rowok and of fetched: its place among the gathered rows, gather_rows).
// R[c] (point-major) = sum_k xs[c]^k Eext[(crow[c] - 1) * N + k] for the complaints c in list[0..cnt)
void cmp_horner(size_t cnt, const uint32_t* list, const uint32_t* xs, const uint32_t* crow, const uint32_t* Eext,
                size_t stride, size_t N, int nb, uint32_t* R, hipStream_t stream);
void cv_prep(size_t C, const uint32_t* party, const uint32_t* pk, const uint32_t* enc, const uint32_t* proofs,
             uint32_t* Pc, uint32_t* rs, uint32_t* nc, uint32_t* p12, uint32_t* bp1, uint32_t* bp2, uint32_t* bq2,
             hipStream_t stream);
void cv_check(size_t C, const uint32_t* accuser, const uint32_t* p12, const uint32_t* ridx, const uint32_t* Rh,
              const uint32_t* Rt, const uint32_t* scale, const uint32_t* tab_g, const uint32_t* tab_h, uint8_t* eq,
              hipStream_t stream);
void cv_final(size_t C, const uint32_t* party, const uint32_t* crow, const uint32_t* pk, const uint32_t* enc,
              const uint32_t* proofs, const uint32_t* a1c, const uint32_t* a2c, const uint8_t* pok, const uint8_t* rowok,
              const uint8_t* fetched, const uint8_t* eq, int32_t* verdict, hipStream_t stream);
void cp_prep(size_t C, const uint32_t* sk, const uint32_t* enc, const uint32_t* w, uint32_t* Pc, uint32_t* ls,
             uint32_t* lb, uint32_t* gs, hipStream_t stream);
void cp_finish(size_t C, const uint32_t* enc, const uint32_t* lc, const uint32_t* gc, const uint32_t* gs,
               uint32_t* proofs, hipStream_t stream);
// qmask[i] = row i of dec [rows][n] holds no MISSING and cmask[i]; rej[i] = !qmask[i]
void qualified_complaints(size_t rows, size_t n, const uint8_t* dec, const uint8_t* cmask, uint8_t* rej, uint8_t* qmask,
                          hipStream_t stream);
// round-4 complaints (MisbehavingPartiesRound3::verify, broadcast.rs:104-144), lane = complaint: the
// reduced scalars sr [2C][8] = (share, randomness) and the evaluation items' lists acc2 / acd2 [2C]
// (item 2c: E row crow - 1, item 2c + 1: A row arows + crow - 1 of the decoded 2 arows rows; one
// ceremony: arows = n, crow = accused);
void c3_prep(size_t C, size_t arows, const uint32_t* accuser, const uint32_t* crow, const uint32_t* share,
             const uint32_t* randomness, uint32_t* sr, uint32_t* acc2, uint32_t* acd2, hipStream_t stream);
// eq[2c] = (g share + h randomness == P^E), eq[2c + 1] = (g share == P^A); ridx [2C], Rh, Rt, scale as cv_check;
void c3_check(size_t C, const uint32_t* accuser, const uint32_t* sr, const uint32_t* ridx, const uint32_t* Rh,
              const uint32_t* Rt, const uint32_t* scale, const uint32_t* tab_g, const uint32_t* tab_h, uint8_t* eq,
              hipStream_t stream);
// the verdicts (rowok [2 arows] by crow; qualified, fetched3, may be null, by the 1-based dealer row drow)
void c3_final(size_t C, size_t arows, const uint32_t* crow, const uint32_t* drow, const uint8_t* rowok,
              const uint8_t* qualified, const uint8_t* fetched3, const uint8_t* eq, int32_t* verdict,
              hipStream_t stream);
// ---- the complaint stage of batched ceremonies (dealer row g n + i = dealer i of ceremony g)
// out [R][N][8] = rows `rows[r]` (0-based dealer rows) of srcE; with srcA, [2R][N][8]: then those of srcA
void gather_rows(size_t R, size_t N, const uint32_t* rows, const uint32_t* srcE, const uint32_t* srcA, uint32_t* out,
                 hipStream_t stream);
// enc [C][32 words] = the pair dealer row drow[c] (1-based) sent recipient accuser[c] of its ceremony,
// from the batch's e1 / ct [V][n][2][8]
void gather_enc(size_t C, size_t n, const uint32_t* drow, const uint32_t* accuser, const uint32_t* e1,
                const uint32_t* ct, uint32_t* enc, hipStream_t stream);
// verdict 0 of a round-2 complaint: cmask[drow2 - 1] = 0, pair[(drow2 - 1) n + accuser2 - 1] = 1; verdict
// 0 or 5 of a round-4 complaint: proven4[drow4 - 1] = 1 (the masks preset by the caller; with C2 == 0
// cmask / pair may be null)
void proven_masks(size_t C2, size_t n, const uint32_t* drow2, const uint32_t* accuser2, const int32_t* verdict2,
                  size_t C4, const uint32_t* drow4, const int32_t* verdict4, uint8_t* cmask, uint8_t* pair,
                  uint8_t* proven4, hipStream_t stream);
// dissent[g n + j] = #{i : dec2[g n + i][j] == REJECT and not pair[g n + i][j]}, V = groups * n
void dissent_rows(size_t V, size_t n, const uint8_t* dec2, const uint8_t* pair, int32_t* dissent, hipStream_t stream);
// out[i] = dok[column of dealer i of segment seg] (and_dealer_mask's layout), i < D
void segment_mask(size_t D, int nseg, int seg, const uint8_t* dok, uint8_t* out, hipStream_t stream);
// ---- the complaint stage of a dealer-sharded rank (its D dealers; lrow = the accused's 1-based local row)
// ridx [items C] of the owned complaints' items as elements of the fused pass's R (bit 31 set; items = 1:
// the E row, 2: E then A), or element 0 of Rh for a complaint with a row that does not decode (rowok [2D])
void shard_ridx(size_t C, int items, size_t D, size_t n, const uint32_t* lrow, const uint32_t* accuser,
                const uint8_t* rowok, uint32_t* ridx, hipStream_t stream);
// flags [rows]: bit 0 !cmask (null: clear), bit 1 proven4, bit 2 !a_dec or !fetched3 (null: present); rows past D zero
void shard_flags(size_t D, size_t rows, const uint8_t* cmask, const uint8_t* proven4, const uint8_t* a_dec,
                 const uint8_t* fetched3, uint32_t* flags, hipStream_t stream);
// dissent[j] = #{i < D : dec2[i][j] == REJECT and not pair[i][j]}
void shard_dissent(size_t D, size_t n, const uint8_t* dec2, const uint8_t* pair, int32_t* dissent, hipStream_t stream);
// flags [n] -> cmask (bit 0 clear), proven4 (bit 1), a_ok (bit 2 clear)
void flag_masks(size_t n, const uint32_t* flags, uint8_t* cmask, uint8_t* proven4, uint8_t* a_ok, hipStream_t stream);
// out[j] = sum_r in[r][j], in [ws][n]
void sum_partials_i32(size_t ws, size_t n, const int32_t* in, int32_t* out, hipStream_t stream);

// ---- committee verification by interpolation (interp.hip)
// F[d][k] = sum_j W[k][j] s[d][j] (and F' from s'; sp may be null), WT[j][k] = W[k][j] in Montgomery form
void interp(size_t D, size_t N, size_t nrecv, const uint32_t* WT, const uint32_t* s, const uint32_t* sp, uint32_t* F,
            uint32_t* Fp, hipStream_t stream);
// per (d, k): okA = (g F_k == A_k), okE = (g F_k + h F'_k == E_k); commitments [D][N] extended
void coef_check(size_t D, size_t N, const uint32_t* F, const uint32_t* Fp, const uint32_t* Eext, const uint32_t* Aext,
                size_t cstride, const uint32_t* tab_g, const uint32_t* tab_h, uint8_t* okE, uint8_t* okA,
                hipStream_t stream);
// round-2 / round-4 decisions of the rows whose coefficient test passed (others: 0, re-verified)
void interp_decide(size_t D, size_t nrecv, size_t N, size_t dealer_base, size_t nmod, const uint32_t* s,
                   const uint32_t* sp, const uint32_t* F, const uint32_t* Fp, const uint8_t* dokE, const uint8_t* dokA,
                   const uint8_t* cE, const uint8_t* cA, const uint32_t* tab_g, const uint32_t* tab_h, uint8_t* dec2,
                   uint8_t* dec4, hipStream_t stream);
// ok[i] &= extra[i], i < D
void and_mask(size_t D, const uint8_t* extra, uint8_t* ok, hipStream_t stream);

// ---- one party's share checks (receivers.hip): P_i(x) for a few receiver indices, chunked Horner
// stage 1: chunks of L coefficients of the position-major table C [40][N][npad] for the Ms index slots
// m0 .. m0 + Ms - 1 of xs (1-based indices): Q [40][Ms][G][npad], G = ceil(N / L); with G == 1 the
// values go to R [(m0 + m) * ndealers + d][40] (point-major) instead
void recv_chunks(size_t ndealers, size_t npad, size_t N, size_t L, const uint32_t* C, const uint32_t* xs, size_t m0,
                 size_t Ms, uint32_t* Q, uint32_t* R, hipStream_t stream);
// one fold stage: groups of r consecutive partials of in [40][Ms][Gin][npad] by Horner in the stage's
// multiplier; digits + (m0 + m) * dstride: NAF +1 bits (8 words), -1 bits (8 words), length.  out
// [40][Ms][ceil(Gin / r)][npad], or R (as recv_chunks) when one value per slot is left
void recv_fold(size_t ndealers, size_t npad, size_t Gin, size_t r, const uint32_t* in, const uint32_t* digits,
               size_t dstride, size_t m0, size_t Ms, uint32_t* out, uint32_t* R, hipStream_t stream);
// dec [M][n] holds check's accept / reject of every pair; rows that do not decode, SELF (i + 1 == xs[m])
// and SKIPPED (qualified, may be null) are applied in place
void recv_decide(size_t M, size_t n, int round, const uint32_t* xs, const uint8_t* dok, const uint8_t* qualified,
                 uint8_t* dec, hipStream_t stream);
// P [M][D][8] = encodings of R [M * D][40], zero where dok[i] == 0
void recv_encode(size_t M, size_t D, const uint32_t* R, const uint8_t* dok, uint32_t* P, hipStream_t stream);
// one wave per (row, index) item: item b is complaint c = list[b] (b with a null list), row crow[c] - 1 of
// the decoded commitments Eext (element row * N + k, stride as cmp_horner), index xs[c]; the wave's lanes
// walk G = ceil(N / L) <= 64 chunks and fold them in S = ceil(log2 G) stages (dkg_pair_eval_shape) with
// the multipliers' records digits[slot[b]][S][17] (NAF +1 bits, -1 bits, length).  R[c][40] point-major
void pair_eval(size_t cnt, const uint32_t* list, const uint32_t* xs, const uint32_t* crow, const uint32_t* slot,
               const uint32_t* Eext, size_t stride, size_t N, uint32_t L, uint32_t G, uint32_t S,
               const uint32_t* digits, uint32_t* R, hipStream_t stream);
// ---- seats (ceremony, party) of one operator: dkg_seat_pack's waves, one workgroup each (k_seat_horner).
// Wave v evaluates at x = wdesc[2v] the dealers wdesc[2v + 1] * 64 + i, i < width (a power of two <= 64),
// of the 64 / width seats wseat[v * (64 / width) + slot] (0xffffffff: empty); seat p reads columns
// scol[p] * n + dealer of the position-major table C [40][N][cols].  R [seat * n + dealer][40] point-major
void seat_horner(size_t waves, size_t n, size_t N, size_t cols, uint32_t width, const uint32_t* wdesc,
                 const uint32_t* wseat, const uint32_t* scol, const uint32_t* C, uint32_t* R, hipStream_t stream);
// The same evaluation cut into G = ceil(N / L) chunks of L coefficients (k_seat_chunks, grid (waves, G))
// and folded in ceil(log2 G) stages of arity 2 (k_seat_fold, one launch per stage).  Q, in, out hold
// partials lanes-minor, [40][chunks][64 * waves]; nothing is launched for G > 65535.  seat_fold: wave v
// multiplies by the 17-word digit record digits[xslot[v] * dstride ..] (y = x^(L 2^stage), as recv_fold's
// records); the stage with Gin <= 2 stores the live lanes to R as seat_horner does, the others to out.
void seat_chunks(size_t waves, size_t n, size_t N, size_t cols, uint32_t width, size_t L, const uint32_t* wdesc,
                 const uint32_t* wseat, const uint32_t* scol, const uint32_t* C, uint32_t* Q, hipStream_t stream);
void seat_fold(size_t waves, size_t n, uint32_t width, size_t Gin, const uint32_t* wdesc, const uint32_t* wseat,
               const uint32_t* xslot, const uint32_t* digits, size_t dstride, const uint32_t* in, uint32_t* out,
               uint32_t* R, hipStream_t stream);
// sok [S][n] = dok[scol[p] * n + i] and extra [S][n] (may be null)
void seat_ok(size_t S, size_t n, const uint32_t* scol, const uint8_t* dok, const uint8_t* extra, uint8_t* sok,
             hipStream_t stream);
// recv_decide per seat: party sx[p] - 1 of ceremony scer[p]; sok [S][n]; qualified [B][n] (may be null)
void seat_decide(size_t S, size_t n, int round, const uint32_t* sx, const uint32_t* scer, const uint8_t* sok,
                 const uint8_t* qualified, uint8_t* dec, hipStream_t stream);
// ok[p] = rowok[crow[p] - 1], p < cnt
void pair_ok(size_t cnt, const uint32_t* crow, const uint8_t* rowok, uint8_t* ok, hipStream_t stream);

// ---- public shares from the broadcast commitments (pubshares.hip; one build, namespace dkgk only)
// Sacc [40][N][bpad] += the column sums of the slab's used rows: the slab holds global rows [r0, r0 + rows)
// decoded position-major, C [40][N][spad] with rowok [rows]; use [B n] over the global rows (null: all
// used): 0 not used, 1 used, 2 used but absent.  ok[c] = 0 where a used row of ceremony c is absent or does
// not decode.  Nothing is launched for spad < rows or a ceremony past bpad.
void commit_colsum(size_t n, size_t N, size_t r0, size_t rows, size_t spad, const uint32_t* C, const uint8_t* rowok,
                   const uint8_t* use, size_t bpad, uint32_t* Sacc, uint8_t* ok, hipStream_t stream);
// V [B][M][8] = encodings of R[m B + c] (point-major) + G[c M + m] (SoA at stride B M; null: nothing added)
void pubshare_out(size_t B, size_t M, const uint32_t* R, const uint32_t* G, uint32_t* V, hipStream_t stream);

}  // namespace dkgk
