/*
 * dkg_amd.h — C ABI of the MI355X (gfx950) backend for the share-generation and
 * share-verification hot path of danielSanchezQ/dkg (Pedersen-VSS DKG over Ristretto255).
 *
 * Encodings (identical to the reference's wire values):
 *   scalar = 32 bytes little-endian, canonical mod l      (groups.rs:23-27); a scalar input that is
 *            not canonical is read as Scalar::from_bytes reads it (from_bits, groups.rs:29-36):
 *            bit 255 is dropped and the rest reduced mod l
 *   point  = 32 bytes compressed Ristretto255             (groups.rs:72-76)
 * Every buffer is caller-owned host memory unless a function name ends in `_device`
 * (then the pointers are HIP device pointers).  No pointer is retained after return.
 * One dkg_ctx drives one GPU (one process per GPU); a ctx is not re-entrant.
 *
 * Status codes: protocol outcomes (a rejected share, MisbehaviourHigherThreshold) are DATA,
 * returned in decision matrices and flags; negative codes are call failures only.
 */
#ifndef DKG_AMD_H
#define DKG_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DKG_OK 0
#define DKG_E_ARG (-1)    /* where the reference panics: length mismatch, t >= (n+1)/2, index range */
#define DKG_E_DECODE (-2) /* an input point does not decode (CompressedRistretto::decompress -> None) */
#define DKG_E_DEVICE (-3) /* HIP runtime failure (message in dkg_ctx_last_error) */
#define DKG_E_NOMEM (-4)

/* decision matrix values ([dealer][receiver], one byte per pair) */
#define DKG_REJECT 0
#define DKG_ACCEPT 1
#define DKG_SELF 2       /* i == j: a party never checks itself (qualified_set starts at 1) */
#define DKG_SKIPPED 3    /* round 4 only: dealer not qualified, check skipped (committee.rs:522) */
#define DKG_MISSING 4    /* round 2 only: the dealer's broadcast does not decode (no data): it is
                          * disqualified WITHOUT a complaint (committee.rs:331-335); in round 4 the
                          * same case is an accusation (:549-555) and reads DKG_REJECT */

typedef struct dkg_ctx dkg_ctx;

/* ---- context ---- */
int dkg_ctx_create(int device, dkg_ctx **out);
void dkg_ctx_destroy(dkg_ctx *ctx);
const char *dkg_ctx_last_error(const dkg_ctx *ctx);
/* Device time (ms) of one phase of the last ceremony's round-2 / round-4 checks, by name
 * "r2.binomial", "r2.stepping", "r2.combine" (degree split only, else 0), "r2.check", "r4.*", or
 * "r24.*" for the fused rounds (HIP events
 * on the ctx stream, recorded only with dkg_ctx_set_streams(ctx, 1)); -1 if unknown. */
double dkg_ctx_phase_ms(const dkg_ctx *ctx, const char *name);
/* Scheduling of the round-2/4 checks: the dealers are cut into nsub chunks (1..8, default 2)
 * whose pipelines run on their own HIP streams and overlap on the GPU.  nsub = 1 serialises
 * them and is the only mode that records dkg_ctx_phase_ms.  Results do not depend on nsub. */
int dkg_ctx_set_streams(dkg_ctx *ctx, int nsub);
/* on != 0 (default): the ceremony drivers verify round 2 (committee.rs:273-338) and round 4
 * (committee.rs:520-559) as ONE fused pipeline over both commitment vectors.  The round-4 inputs
 * (A_i, s_ij) are fixed in round 1 and only the SKIPPED mask of disqualified dealers depends on
 * round 2 (it is applied afterwards), so every output is identical to protocol order; ms_round2
 * then covers both rounds' checks and ms_round4 only the copy-back.  on == 0: protocol order.
 * Phase times (dkg_ctx_phase_ms, nsub == 1) are recorded under "r24.*" when fused. */
int dkg_ctx_set_overlap(dkg_ctx *ctx, int on);
/* Degree split of the difference tables: pieces = U > 1 evaluates the
 * committed polynomial as U pieces of degree < ceil((t+1)/U) recombined per receiver with U-1
 * multiplications by j^L; 0 (default) picks U with the cost model dkg_split_model_ms; 1 disables.
 * Decisions and outputs do not depend on it. */
int dkg_ctx_set_split(dkg_ctx *ctx, int pieces);
/* How the stepping covers its tables: 0 (default) by the cost model; 1 one workgroup slot per
 * column holding all its pieces (split tables whose pieces fit one 512-lane workgroup); 2 one slot
 * per piece; 3 as 0 without the dead-position repack of short unsplit tables (DESIGN.md section 4:
 * the last steps on halved segments once the top positions stop adding).  Outputs do not depend
 * on it. */
int dkg_ctx_set_stepping(dkg_ctx *ctx, int mode);
/* Field multiplication of the verification kernels: 0 (default) per launch by occupancy, 1 always
 * product scanning (fewest issue slots), 2 always column sums (most independent chains; for
 * latency-bound launches).  Outputs do not depend on it. */
int dkg_ctx_set_field_mode(dkg_ctx *ctx, int mode);
/* Schedule of the binomial-basis Horner: 0 (default) -- tables of many column
 * groups (config 5) as ONE launch in which every wave runs all steps of its 64 columns in place,
 * others one grid launch per step with the steps under one wave per SIMD on lane pairs (each point
 * on two lanes sharing its field products); 1 -- per step, no lane pairs; 2 -- per step, lane pairs
 * for every step; 3 -- per step as 0's; 4 -- per wave always; 5 -- per wave always, each item's
 * operand loaded during the previous item's chain.  Outputs do not depend on it. */
int dkg_ctx_set_binomial(dkg_ctx *ctx, int mode);
/* The fused round-2/4 checks (g*s compared in round 4, + h*s' in round 2): 0 (default) one launch
 * reading both fixed-base combs; 1 two launches that each read one comb, g*s parked in device memory
 * between them.  Mode 1 dates from the radix-2^11 combs (3.1 MB per base, one XCD's 4-MB L2 held
 * one); the radix-2^19 combs (470 MB per base, HBM / Infinity Cache) leave it no cache to win, and
 * it stays as an A/B option.  Outputs do not depend on it. */
int dkg_ctx_set_check(dkg_ctx *ctx, int mode);
/* Verification algorithm of the ceremony drivers (all-receivers views: dkg_ceremony_*, batch, shard):
 *  0 (default) -- difference tables: every P_i(j) = sum_k j^k C_k is computed as a group element and
 *                 compared with g s_ij + h s'_ij, as each receiver of the reference does;
 *  1           -- committee verification by interpolation: the shares at receivers 1..t+1 fix the
 *                 dealer's scalar polynomials F, F' (inverse Vandermonde); its commitments are
 *                 tested once against g F_k + h F'_k, and each remaining pair reduces to comparing
 *                 s_ij with F(j) (a deviating share is decided by its own group equation); rows
 *                 whose commitments are not of that form are re-verified with mode 0.  Every
 *                 decision equals mode 0's.  Needs all n shares of a dealer,
 *                 so dkg_verify_receiver (one party's column) always uses its own path. */
int dkg_ctx_set_verify_mode(dkg_ctx *ctx, int mode);
/* Mode 1: rows of the last verification that were re-verified with difference tables. */
size_t dkg_ctx_fallback_rows(const dkg_ctx *ctx);
/* U used by the last ceremony's checks on this ctx. */
int dkg_ctx_last_split(const dkg_ctx *ctx);
/* Piece length L of that split: pieces 0..U-2 hold L coefficients, the last one t+1-(U-1)L. */
size_t dkg_ctx_last_split_len(const dkg_ctx *ctx);
/* The cost model's estimate (ms) of binomial + recombination for `columns` difference tables. */
double dkg_split_model_ms(size_t columns, size_t n, size_t t, int pieces);
/* The piece length L the runtime uses for a `pieces`-way split of such tables (0 on bad input). */
size_t dkg_split_len(size_t columns, size_t n, size_t t, int pieces);
/* Recombination of a degree split: 0 (default) short multipliers for 2..5 pieces (2..4 with
 * projective addends) -- receiver j's pieces are combined as b_j P(j) = b_j Q_0(j) + a_j1 Q_1(j) + ..
 * with a short lattice vector (b_j, a_j1, ..), a_ju = b_j j^(uL) mod l (126 / 168 / 189 / 202-bit
 * scalars for 2 / 3 / 4 / 5 pieces instead of 253), and the checks compare with g*(b_j s) +
 * h*(b_j s'); 1 powers of y = j^L (253-bit
 * NAFs, pairwise Horner in y^2, any number of pieces); 2 = 0; 3 short multipliers with one NAF per
 * scalar at every piece count.  With 2 or 4 pieces and affine addends, modes 0 and 2 recode the
 * pairs (0,1), (2,3) in joint sparse form and add a pair's sum or difference, streamed from memory,
 * where both digits are set (190 instead of 254 additions per item at 4 pieces); mode 3 keeps the
 * per-scalar chains there too.  dkg_split_multipliers returns the rows of mode 0.  Decisions do not
 * depend on it. */
int dkg_ctx_set_combine(dkg_ctx *ctx, int mode);
/* What the last verification recombined with: 0 no split, 1 powers of y, 2 short multipliers. */
int dkg_ctx_last_combine(const dkg_ctx *ctx);
/* How the last verification ran its binomial: 0 one launch per Horner step, 1 per-wave loops
 * (k_binom_wave, one launch per chunk stream). */
int dkg_ctx_last_binomial(const dkg_ctx *ctx);
/* Addends of the short-multiplier recombination: 0 (default) affine Niels (the stepped values
 * normalised with one inversion per run of receivers; mixed additions, 7M instead of 8M), 1 cached
 * projective.  Outputs do not depend on it. */
int dkg_ctx_set_addends(dkg_ctx *ctx, int mode);
/* Additions of the finite-difference stepping: 0 (default) the dedicated formula (HWCD 2008, no
 * product by d; not complete), with every workgroup that met an exceptional pair (a sum with Z = 0:
 * equal or 2-/4-torsion-related points, which crafted commitments can reach) recomputed by the
 * complete formula; 1 the complete formula only.  Outputs do not depend on it. */
int dkg_ctx_set_stepping_formula(dkg_ctx *ctx, int mode);
/* Workgroups of the last verification's stepping that were recomputed by the complete formula
 * (synchronises the context's stream; 0 in mode 1; -1 on error). */
long long dkg_ctx_stepping_redos(dkg_ctx *ctx);
/* Test aid: the device's zero tests of a field product (fe25519.h) on count elements of ten 32-bit
 * limbs each, limbs [count][10]: out [count][3] = the one-limb filter (fe_maybe_zero), the full test
 * (fe_tight_zero), and the filtered guard the dedicated additions use (fe_zero_guard), each 0 or 1.
 * The guard equals the full test on every input. */
int dkg_zero_tests(dkg_ctx *ctx, size_t count, const uint32_t *limbs, uint8_t *out);
/* Test aid: one field primitive (fe25519.h) on count operand tuples of raw 32-bit limb words, one tuple
 * per lane; results are limbs too, so their bounds can be checked.  flavour as dkg_ctx_set_field_mode:
 * 1 product scanning, 2 column sums.  op, with the words per tuple in -> out (an element is ten limbs):
 *   0 fe_mul (f, g) 20 -> 10          1 fe_sq 10 -> 10
 *   2 fe_mul2 (fa, ga, fb, gb) 40 -> 20 (ra, rb)      3 fe_sq2 (fa, fb) 20 -> 20
 *   4 fe_mul_small (a, k < 2^12) 11 -> 10             5 fe_carry 10 -> 10
 *   6 fe_add (a, b) 20 -> 10          7 fe_sub (a, b) 20 -> 10
 *   8 fe_neg 10 -> 10                 9 fe_dbl 10 -> 10
 *  10 fe_invert 10 -> 10             11 fe_pow22523 10 -> 10
 *  12 fe_tobytes32 10 -> 10: the 8 words, fe_isneg, fe_iszero
 *  13 fe_frombytes32 8 -> 10         14 fe_abs 10 -> 10
 * The operands must lie in the primitive's documented range.  DKG_E_ARG for an unknown op or flavour;
 * count == 0 touches nothing. */
int dkg_fe_ops(dkg_ctx *ctx, int flavour, int op, size_t count, const uint32_t *in, uint32_t *out);
/* Test aid: one scalar primitive (sc25519.h) on count operand tuples of 32-bit little-endian words, one
 * per lane (a scalar is 8 words).  op, with the words per tuple in -> out:
 *   0 sc_reduce9 9 -> 8               1 sc_reduce256 8 -> 8           2 sc_reduce512 16 -> 8
 *   3 sc_add (a, b) 16 -> 8           4 sc_sub (a, b) 16 -> 8         5 sc_neg 8 -> 8
 *   6 sc_mul_small_add (a, x, c) 17 -> 8              7 sc_horner2 (a, x, c1, c0) 25 -> 8
 *   8 the lazy accumulator (state [10], steps <= 5, x, coefficient [8]) 20 -> 18: `steps` calls of
 *     sc_lazy_step, then sc_lazy_fold; the folded state [10] and sc_lazy_final [8]
 *   9 sc_mont_mul (a, b) 16 -> 8     10 sc_mul (a, b) 16 -> 8        11 sc_mont_inv 8 -> 8
 *  12 sc_radix16 8 -> 16: the 64 signed digits as bytes, four to a word
 * DKG_E_ARG for an unknown op or too many lazy steps; count == 0 touches nothing. */
int dkg_sc_ops(dkg_ctx *ctx, int op, size_t count, const uint32_t *in, uint32_t *out);
/* The stepping's banded lane map ("Dead positions"): a `lanes`-lane workgroup
 * made of slots of `nseg` segments, `seg_len` lanes each except a slot's last (`last_len`).  Returns
 * the band width B (wave w holds positions [wB, (w+1)B) of every segment) and fills out[0..2] with
 * lane `lane`'s segment, its position there and the lane that holds the next position; returns 0,
 * out untouched, when such a workgroup keeps 64 consecutive positions per wave, -1 on bad input. */
int dkg_stepping_lane_map(int lanes, int seg_len, int nseg, int last_len, int lane, int out[3]);
/* 1 when the last single-ceremony or dealer-shard call reran its verification with the complete
 * formula because a dedicated addition of the per-step binomial met Z = 0 (an exceptional pair, e.g.
 * a crafted all-identity commitment row), else 0 (-1 on a NULL ctx). */
int dkg_ctx_binomial_reruns(dkg_ctx *ctx);
/* Test aid: the (piece, 64-column group) flag words that the last verification's per-wave binomial
 * (k_binom_wave) marked -- a dedicated addition of a real column met Z = 0 there -- and rebuilt with the
 * complete formula (synchronises the context's stream; 0 when the complete formula or the per-step
 * binomial ran; -1 on error).  Read after the call: the timed paths do nothing for it. */
long long dkg_ctx_binomial_wave_redos(dkg_ctx *ctx);
/* The short multipliers (b_j, a_j1, .., a_j(U-1)) of receivers j = 1..n for a `pieces`-way split of
 * piece length L (2 <= pieces <= 5): magnitudes mag[n][pieces][32] (little-endian), signs
 * sign[n][pieces] (+1 / -1); a_ju = b_j j^(uL) mod l and b_j > 0.  DKG_E_ARG on bad input. */
int dkg_split_multipliers(size_t n, size_t L, int pieces, uint8_t *mag, int8_t *sign);
/* Solinas' joint sparse form of two 256-bit magnitudes (32 bytes little-endian each): digits
 * da[256], db[256] in {-1, 0, 1} with sum da[i] 2^i = a and sum db[i] 2^i = b, a zero column among
 * any three consecutive positions and the fewest nonzero columns; *top = the highest position with a
 * nonzero digit (-1: both inputs zero).  DKG_E_ARG if the form does not fit 256 positions (only
 * inputs of 2^255 or more can carry out).  Host-only. */
int dkg_jsf_digits(const uint8_t a[32], const uint8_t b[32], int8_t da[256], int8_t db[256], int16_t *top);
/* The signed chain digits digits[n][pieces][256] and top[n] that recombination mode `mode` (0, 2 or
 * 3, see dkg_ctx_set_combine) runs for that split: pairs (0,1), (2,3) in joint sparse form where the
 * pairwise chain is built (2 and 4 pieces, modes 0 and 2), NAFs otherwise; each scalar's sign is
 * applied to its digits, and the rows are those the mode selects.  Host-only. */
int dkg_split_digits(size_t n, size_t L, int pieces, int mode, int8_t *digits, int16_t *top);
/* Number of GPUs visible to this process (counts only; does not create a context). */
int dkg_device_count(void);
/* Measurement aids (bench.py; no reference counterpart).
 * dkg_ctx_clock_probe: 4 waves per SIMD on every CU of the ctx's device each run `iters` dependent
 * VALU iterations, reading the shader clock (s_memtime) and the constant-rate clock (s_memrealtime,
 * hipDeviceAttributeWallClockRate) around them; *sclk_mhz = the median over waves of shader cycles
 * per real-time microsecond (the clock the VALU ran at under full occupancy), *busy_ms = the
 * probe's real-time span (median).  dkg_device_pci_bus_id: the device's PCI bus id
 * ("dddd:bb:dd.f", hipDeviceGetPCIBusId) into buf[len]. */
int dkg_ctx_clock_probe(dkg_ctx *ctx, unsigned iters, double *sclk_mhz, double *busy_ms);
int dkg_device_pci_bus_id(int device, char *buf, int len);

/* ---- Environment::init (committee.rs:72-83) ----
 * Checks threshold < (nr_members + 1) / 2 (DKG_E_ARG otherwise, where the reference asserts) and
 * derives the Pedersen commitment key h = hash_to_group::<Blake2b>(ck_bytes) (commitment.rs:13-17),
 * caching its fixed-base table on the device.  h_out may be NULL. */
int dkg_env_init(dkg_ctx *ctx, size_t threshold, size_t nr_members, const uint8_t *ck_bytes, size_t ck_len,
                 uint8_t h_out[32]);
/* Same check without a context (pure function). */
int dkg_env_check(size_t threshold, size_t nr_members);

/* ---- trait-level batches (traits.rs:142-238, groups.rs:11-90) ---- */
/* PrimeGroupElement::vartime_multiscalar_multiplication (traits.rs:234-237), B independent MSMs of
 * N terms: out[b] = sum_k scalars[b][k] * points[b][k].  scalars [B][N][32], points [B][N][32]. */
int dkg_msm_batch(dkg_ctx *ctx, size_t B, size_t N, const uint8_t *scalars, const uint8_t *points, uint8_t *out);
/* Mul<Scalar> by a fixed base (traits.rs:212): out[c] = scalars[c] * base.  base == NULL means
 * PrimeGroupElement::generator() (groups.rs:60-62). */
int dkg_fixed_base_batch(dkg_ctx *ctx, const uint8_t base[32], size_t count, const uint8_t *scalars, uint8_t *out);
/* Polynomial::evaluate (polynomial.rs:68-74) of D polynomials with N coefficients each
 * (coeffs [D][N][32]) at M small integer points xs[m] < 2^24: out [D][M][32]. */
int dkg_poly_eval_batch(dkg_ctx *ctx, size_t D, size_t N, const uint8_t *coeffs, size_t M, const uint32_t *xs,
                        uint8_t *out);
/* PrimeGroupElement::from_bytes validity (groups.rs:78-81): ok[c] = 1 iff points[c] decodes. */
int dkg_points_valid_batch(dkg_ctx *ctx, size_t count, const uint8_t *points, uint8_t *ok);

/* ---- round 1: share generation (Phases<Initialise>::init, committee.rs:124-216) ----
 * For dealers i in [0, D): coefficients a (sharing) and b (hiding), [D][t+1][32];
 * E[i][k] = h*b[i][k] + g*a[i][k], A[i][k] = g*a[i][k] ([D][t+1][32], committee.rs:151-159);
 * s[i][j] = f_i(j+1), s_prime[i][j] = f'_i(j+1) for receivers j in [0, n) ([D][n][32], :164-167).
 * Requires dkg_env_init (for h).  Any output may be NULL to skip it. */
int dkg_share_gen(dkg_ctx *ctx, size_t D, size_t n, size_t t, const uint8_t *a, const uint8_t *b, uint8_t *E,
                  uint8_t *A, uint8_t *s, uint8_t *s_prime);
/* The same on device buffers (canonical scalars d_a, d_b [D][t+1][32] in; d_E, d_A [D][t+1][32]
 * compressed -- either may be NULL -- and d_s, d_s_prime [D][n][32] out), e.g. to build the
 * broadcasts of a large committee in HBM for dkg_ceremony_shard_verify_device. */
int dkg_share_gen_device(dkg_ctx *ctx, size_t D, size_t n, size_t t, const void *d_a, const void *d_b, void *d_E,
                         void *d_A, void *d_s, void *d_s_prime);

/* ---- rounds 2 and 4: share checks ----
 * round 2 (Phases<Phase1>::proceed, committee.rs:273-338): h*s' + g*s == sum_k (j+1)^k E_i[k]
 * round 4 (Phases<Phase3>::proceed, committee.rs:520-559):          g*s == sum_k (j+1)^k A_i[k]
 * for dealers i in [d0, d1) and ALL receivers j in [0, n).  C = E (round 2) or A (round 4) of those
 * dealers, [d1-d0][t+1][32]; s, s_prime = the dealers' share rows [d1-d0][n][32] (s_prime unused in
 * round 4).  decision [d1-d0][n] (DKG_ACCEPT / DKG_REJECT / DKG_SELF).  A dealer whose commitment
 * vector does not decode reads DKG_MISSING for every receiver in round 2 (disqualified without a
 * complaint, committee.rs:331-335) and DKG_REJECT in round 4 (:549-555); the call returns DKG_OK. */
int dkg_verify_pairs(dkg_ctx *ctx, size_t n, size_t t, int round, size_t d0, size_t d1, const uint8_t *C,
                     const uint8_t *s, const uint8_t *s_prime, uint8_t *decision);
/* The same check seen from ONE receiver j (what one party runs in the reference): decisions of
 * receiver j (0-based; index j+1) over all n dealers.  C [n][t+1][32], s / s_prime [n][32] = the
 * column of shares addressed to j.  decision [n]. */
int dkg_verify_receiver(dkg_ctx *ctx, size_t n, size_t t, int round, size_t j, const uint8_t *C, const uint8_t *s,
                        const uint8_t *s_prime, uint8_t *decision);

/* ---- one party's view on the whole device: chunked evaluation (receivers.hip) ----
 * dkg_verify_receiver walks the t + 1 coefficients of every dealer as one dependent chain.  The calls
 * below cut P_i(x) = sum_k x^k C_i[k] into ceil((t+1) / chunk) chunks that are walked side by side
 * (Q_u = sum_{k < chunk} x^k C_i[u chunk + k]) and fold the partials in stages: stage s combines groups
 * of arity[s] consecutive partials by Horner in mult[s].  Every multiplier is one integer for all
 * dealers.  A multiplier may be any representative of its class mod l: the operands lie in 2E, so the
 * results differ by an element of E[4] at most -- the same Ristretto element, encoding and decision. */
typedef struct {
  uint32_t chunk;        /* L >= 1; chunk >= t+1: one chunk, the serial walk (k_horner), stages == 0 */
  uint32_t stages;       /* <= 16 */
  uint32_t arity[16];    /* r_s >= 2: stage s folds groups of r_s consecutive partials */
  uint8_t mult[16][32];  /* y_s, little-endian, < 2^255: y_0 = x^chunk, y_{s+1} = y_s^{r_s} (mod l) */
} dkg_receiver_plan;
/* The plan the runtime executes for receiver index x (1-based, = j + 1) of n parties at threshold t.
 * chunk: 0 = the automatic choice for (n, t, x) -- the cheapest, by a fitted cost rule (chain length x
 * latency + work / throughput + launches), of the serial walk and the chunks 2, 4, .., 64 whose chain
 * is no longer than the serial one; >= 1 forced.  Host only, no GPU, a pure function.  DKG_E_ARG for
 * x == 0, x > n, n == 0, chunk < 0, a NULL out, or a forced chunk that needs more than 16 stages.  It
 * does NOT apply dkg_env_check's t < (n + 1) / 2: any t is planned. */
int dkg_receiver_plan_for(size_t n, size_t t, uint32_t x, int chunk, dkg_receiver_plan *out);
/* The rule's estimate (us) of the evaluation of one index under plan p, and its fitted constants
 * c = {per launch us, per dependent point operation us, per lane and operation us, per dependent
 * operation of the serial walk us, host-side setup of a plan with fold stages us}. */
double dkg_receiver_plan_cost_us(size_t n, size_t t, uint32_t x, const dkg_receiver_plan *p);
void dkg_receiver_plan_constants(double c[5]);
/* Chunk length of the calls below: 0 (default) automatic, >= 1 forced.  Outputs do not depend on it.  It
 * also governs the wave evaluator (dkg_commitment_eval_pairs, dkg_ctx_set_complaint_eval(4)) as
 * dkg_pair_eval_shape's chunk: there a forced chunk that needs more than 64 lanes is DKG_E_ARG. */
int dkg_ctx_set_receiver_chunk(dkg_ctx *ctx, int chunk);
/* The chunk of the last such call's plan (the largest over its indices). */
int dkg_ctx_last_receiver_chunk(const dkg_ctx *ctx);
/* P[m][i] = sum_k (js[m]+1)^k C_i[k], compressed; the shared-scalar case of
 * vartime_multiscalar_multiplication (committee.rs:287-296, 532-539).  C [D][t+1][32]; js[m] < 2^24
 * (DKG_E_ARG otherwise); ok[i] (may be NULL) = 0 and P[m][i] = 32 zero bytes where row i does not
 * decode.  P [M][D][32].  Needs no dkg_env_init.  Phase times (dkg_ctx_phase_ms, one stream):
 * "recv.decode" (upload, decode, transposition), "recv.chunks", "recv.fold" (-1, and recv.chunks the
 * whole evaluation, when the indices run as several plans or slabs). */
int dkg_commitment_eval(dkg_ctx *ctx, size_t D, size_t t, size_t M, const uint32_t *js, const uint8_t *C,
                        uint8_t *P, uint8_t *ok);
/* ---- (row, index) pairs, one wave each (receivers.hip k_pair_eval) ----
 * The shape the pair evaluation runs for threshold t: the t + 1 coefficients of one row are cut into
 * `lanes` <= 64 chunks of L that the 64 lanes of one wave walk side by side, and folded in `stages` =
 * ceil(log2 lanes) in-wave stages with the multipliers of dkg_receiver_plan_for(.., chunk = L) (arity 2).
 * chunk: 0 = automatic, L = ceil((t+1) / 64); >= 1 forced (a chunk >= t + 1 reads L = t + 1: one lane, no
 * stage).  Host only, no GPU, a pure function.  DKG_E_ARG for a forced chunk that needs more than 64
 * lanes, chunk < 0 or a NULL output. */
int dkg_pair_eval_shape(size_t t, int chunk, uint32_t *L, uint32_t *lanes, uint32_t *stages);
/* P[p] = sum_k (js[p]+1)^k C_rows[p][k], compressed: vartime_multiscalar_multiplication for a LIST of
 * (row, index) pairs (broadcast.rs:75-86, 105-135).  C [D][t+1][32]; rows[p] < D, js[p] < 2^24 (DKG_E_ARG
 * otherwise), any order, repeats allowed.  ok[p] (may be NULL) = 0 and P[p] = 32 zero bytes where row
 * rows[p] does not decode.  Only the DISTINCT rows named are decoded.  count == 0: DKG_OK, nothing
 * touched.  Needs no dkg_env_init.  dkg_ctx_set_receiver_chunk applies (dkg_pair_eval_shape's chunk; a
 * chunk it rejects is DKG_E_ARG here); dkg_ctx_last_receiver_chunk reports the L that ran.  Phases:
 * "pairs.decode", "pairs.eval". */
int dkg_commitment_eval_pairs(dkg_ctx *ctx, size_t D, size_t t, size_t count, const uint32_t *rows,
                              const uint32_t *js, const uint8_t *C, uint8_t *P, uint8_t *ok);
/* dkg_verify_receiver for M receiver indices js[] (0-based, any order, repeats allowed) in one call:
 * s, s_prime [M][n][32] (column m = the shares addressed to js[m]); decision [M][n] with the values
 * of dkg_verify_pairs (SELF where i == js[m], MISSING / REJECT for an undecodable row).  qualified
 * (round 4 only, may be NULL): [n], 0 marks DKG_SKIPPED (committee.rs:522).  Phase-1/Phase-3 proceed
 * of the parties js[] (committee.rs:273-338, 520-559).  M == 0 returns DKG_OK and touches nothing;
 * round 2 requires dkg_env_init.  Also records "recv.check".  With M > 1 and the automatic chunk, every
 * index runs the plan forced to the largest of the indices' automatic chunks (one shape, shared
 * launches); dkg_ctx_last_receiver_chunk reports it. */
int dkg_verify_receivers(dkg_ctx *ctx, size_t n, size_t t, int round, size_t M, const uint32_t *js, const uint8_t *C,
                         const uint8_t *s, const uint8_t *s_prime, const uint8_t *qualified, uint8_t *decision);
/* Phases<Phase1>::proceed (committee.rs:260-366) for ONE party j in full mode: decrypt the n ciphertext
 * pairs addressed to j (e1, ct [n][2][32], w = 0 the randomness, 1 the share) with sk_j, check them
 * against E, and, if w [n][64] is given, ProofOfMisbehaviour::generate (broadcast.rs:189-226) for every
 * REJECT (proofs [n][192], required with w, untouched rows zero).  s_out, sp_out [n][32], complaints,
 * r2_error may be NULL; dec [n]; *complaints = the REJECTs; *r2_error = complaints > t (:340-347).  An
 * e1 that does not decode is missing data (MISSING, no complaint).  Requires dkg_env_init and
 * dkg_env_check(t, n).  Also records "recv.decrypt" and "recv.prove". */
int dkg_party_round2(dkg_ctx *ctx, size_t n, size_t t, size_t j, const uint8_t *E, const uint8_t *e1, const uint8_t *ct,
                     const uint8_t sk[32], const uint8_t *w, uint8_t *s_out, uint8_t *sp_out, uint8_t *dec,
                     int32_t *complaints, uint8_t *r2_error, uint8_t *proofs);

/* ---- hosted seats: one operator's share checks across many ceremonies (receivers.hip k_seat_horner,
 * DESIGN.md section 4) ----
 * A seat is (ceremony c, party j): an operator that holds one party index in each of many ceremonies of
 * one (n, t) runs Phases<Phase1>::proceed and Phases<Phase3>::proceed (committee.rs:260-366, 508-580) for
 * its own index in each.  Every polynomial of a seat is evaluated at x = j + 1, so seats of equal x share
 * a wave with a wave-uniform multiplier.  dkg_seat_pack is that placement, a pure host function that the
 * calls below execute as returned: seats are grouped by x ascending, keep caller order inside a group and
 * fill waves of per_wave slots (a group's last wave may be partly filled; a wave never holds two x); a
 * seat with n > 64 takes `tiles` consecutive waves of 64 dealers.  width W = 64 for n >= 64, else the
 * power of two >= n; per_wave = 64 / W; tiles = ceil(n / 64); wave_of [S] the first wave of seat p,
 * slot_of [S] its slot (< per_wave), *waves the total.  Lane slot * W + i of wave wave_of[p] + tile is
 * dealer tile * 64 + i of seat p, live where that is < n.  DKG_E_ARG for n == 0, js[p] >= n, a NULL js or
 * output with S > 0, or more than 2^32 - 1 waves; S == 0: DKG_OK, *waves = 0 (width, per_wave and tiles
 * are written whenever they are given). */
int dkg_seat_pack(size_t n, size_t S, const uint32_t *js, uint32_t *width, uint32_t *per_wave, uint32_t *tiles,
                  uint32_t *wave_of, uint32_t *slot_of, uint32_t *waves);
/* The three calls share: B ceremonies of (n, t); seat p is party js[p] < n of ceremony cer[p] < B
 * (DKG_E_ARG otherwise), any order, several seats per ceremony and repeats allowed; C (E, A) is
 * [B * n][t+1][32] as in the batch calls, row c * n + i dealer i of ceremony c.  Only the DISTINCT
 * ceremonies named are decoded; rows of other ceremonies are never interpreted.  S == 0 returns DKG_OK and
 * touches nothing.  dkg_ctx_set_field_mode selects the kernel copy.  Phase times (dkg_ctx_phase_ms, one
 * stream): "seats.decrypt", "seats.decode" (upload, gather, decode, transposition), "seats.eval",
 * "seats.check", "seats.prove"; a phase the call did not run reads -1.
 *
 * dkg_commitment_eval with M = 1 per seat (committee.rs:287-296, 532-539): P[p][i] = sum_k (js[p]+1)^k
 * C_{cer[p], i}[k], compressed, [S][n][32]; ok [S][n] (may be NULL) = 0 and P = 32 zero bytes where the
 * row does not decode.  Needs no dkg_env_init. */
int dkg_commitment_eval_seats(dkg_ctx *ctx, size_t B, size_t n, size_t t, size_t S, const uint32_t *cer,
                              const uint32_t *js, const uint8_t *C, uint8_t *P, uint8_t *ok);
/* dkg_verify_receivers with M = 1 per seat (committee.rs:273-338, 520-559): s, s_prime [S][n][32] = the
 * shares addressed to seat p; decision [S][n]; qualified (round 4 only, may be NULL) [B][n], 0 marks
 * DKG_SKIPPED for the seats of that ceremony (:522).  Undecodable row: MISSING (round 2) / REJECT
 * (round 4), then SKIPPED, then SELF.  Round 2 requires dkg_env_init. */
int dkg_verify_seats(dkg_ctx *ctx, size_t B, size_t n, size_t t, int round, size_t S, const uint32_t *cer,
                     const uint32_t *js, const uint8_t *C, const uint8_t *s, const uint8_t *s_prime,
                     const uint8_t *qualified, uint8_t *decision);
/* dkg_party_round2 per seat (Phases<Phase1>::proceed in full mode, committee.rs:260-366): e1, ct
 * [S][n][2][32] = the pairs addressed to seat p, sk [S][32] its keys, w [S][n][64] or NULL; s_out, sp_out
 * [S][n][32], complaints [S], r2_error [S] (may be NULL); dec [S][n]; proofs [S][n][192] (required with
 * w, untouched rows zero).  One decryption launch set for all seats; the REJECTs of all seats are proven
 * in one run.  Requires dkg_env_init and dkg_env_check(t, n). */
int dkg_party_round2_seats(dkg_ctx *ctx, size_t B, size_t n, size_t t, size_t S, const uint32_t *cer,
                           const uint32_t *js, const uint8_t *E, const uint8_t *e1, const uint8_t *ct,
                           const uint8_t *sk, const uint8_t *w, uint8_t *s_out, uint8_t *sp_out, uint8_t *dec,
                           int32_t *complaints, uint8_t *r2_error, uint8_t *proofs);
/* ---- hosted seats of large committees: chunked evaluation (receivers.hip k_seat_chunks, k_seat_fold;
 * DESIGN.md section 4) ----
 * k_seat_horner walks the t + 1 coefficients of a seat's polynomials as one dependent chain (the
 * shared-scalar case of vartime_multiscalar_multiplication, committee.rs:287-296 and :532-539).  A few
 * seats of a large committee leave the device empty behind that chain, so the three calls above may
 * instead cut every polynomial into G = ceil((t+1) / L) chunks that dkg_seat_pack's waves walk side by
 * side (grid waves x G) and fold the partials in `stages` = ceil(log2 G) launches of arity 2 with the
 * multipliers of dkg_receiver_plan_for(n, t, x, L), one digit record per (distinct x, stage).  The
 * placement, the decode and everything after the evaluation are unchanged, and so is the exactness note
 * of the chunked plan above: a multiplier may be any representative mod l.
 *
 * The shape for `waves` waves of dkg_seat_pack whose largest index is x_max (1-based).  chunk >= 1
 * forced: L = min(chunk, t+1), G, stages as dkg_receiver_plan_for's; chunk 0 automatic: the cheapest, by
 * the fitted rule of dkg_receiver_plan_cost_us with 64 * waves lanes and the chain taken at x_max, of the
 * serial walk (L = t+1, G = 1, stages = 0) and L = 2, 4, .., 64 < t+1 whose chain is no longer than the
 * serial one and whose scratch is at most 1 GiB.  *scratch_bytes = 2 * 160 * G * 64 * waves (the partials
 * and their ping-pong partner), 0 for G = 1.  Host only, no GPU, a pure function.  DKG_E_ARG for n == 0,
 * waves == 0, x_max == 0 or > n, chunk < 0, a NULL output, or a forced chunk with G > 65535 (the launch
 * grid; more than 16 stages cannot occur below that). */
int dkg_seat_eval_shape(size_t n, size_t t, size_t waves, uint32_t x_max, int chunk, uint32_t *L, uint32_t *G,
                        uint32_t *stages, uint64_t *scratch_bytes);
/* The rule's fitted constants (profiles/seat_chunks_time.json), c = {per launch us, per dependent point
 * operation of the chunked kernels us, per lane and operation us, per dependent operation of
 * k_seat_horner us, setup of a chunked call us, margin}: a chunked shape is chosen only where its
 * estimate is below margin x the serial walk's (the estimates miss the record by up to a quarter). */
void dkg_seat_eval_constants(double c[6]);
/* The evaluation of the three seats calls: 1 = the serial walk (k_seat_horner); 2 = chunked with
 * dkg_seat_eval_shape(.., chunk) -- a shape that resolves to G = 1 runs the serial kernel and reports 1,
 * one above 1 GiB of scratch is DKG_E_ARG at the call, dkg_ctx_last_error naming the size; 0 (default) =
 * automatic, the rule with chunk 0.  chunk is read in mode 2 only and must be 0 otherwise.  Outputs never
 * depend on mode or chunk.  dkg_ctx_set_field_mode selects the kernel copy of either route;
 * dkg_ctx_set_receiver_chunk does not apply to seats.  A chunked call on one stream also records
 * "seats.fold", the fold stages alone (inside "seats.eval"); -1 otherwise.  DKG_E_ARG for any other
 * mode, chunk < 0, or chunk != 0 outside mode 2. */
int dkg_ctx_set_seat_eval(dkg_ctx *ctx, int mode, int chunk);
/* The route (1 or 2) the last seats call ran and, in *chunk (may be NULL), its L (t + 1 for the serial
 * walk); 0 and 0 before the first. */
int dkg_ctx_last_seat_eval(const dkg_ctx *ctx, int *chunk);

/* ---- hosted seats deal round 1 (seat_deal.hip) ----
 * Phases<Initialise>::init (committee.rs:124-216) for every seat of an operator in one call: seat p, party
 * js[p] of ceremony cer[p] (the seats calls' rules above), commits to its two polynomials a[p], b[p]
 * ([S][t+1][32] sharing / hiding coefficients), evaluates the n shares and randomness values and
 * hybrid-encrypts both to ALL n members of its ceremony, itself included (:164-178), under r
 * ([S][n][2][32], w = 0 the randomness s', 1 the share s; read reduced mod l).  pk [B][n][32] the sorted
 * member keys per ceremony.  Output row p equals, byte for byte, dkg_share_gen(D = 1) on (a[p], b[p])
 * followed by dkg_encrypt_shares(D = 1) to pk[cer[p]] with r[p]: E, A [S][t+1][32]; e1, ct [S][n][2][32]
 * (the EncryptedShares of BroadcastPhase1); s_out, sp_out [S][n][32] (may be NULL); own [S][2][32] (may be
 * NULL) = (s', s) at js[p], what init keeps as decrypted_shares[my - 1] (:179-185).
 * Only the DISTINCT ceremonies named are decoded: a key set no seat names is never interpreted.  A key of
 * a named ceremony that does not decode: DKG_E_DECODE, dkg_ctx_last_error names the ceremony and the
 * recipient, the outputs are unspecified.  S == 0 returns DKG_OK and touches nothing.  Requires
 * dkg_env_init (h) and dkg_env_check(t, n); DKG_E_ARG for B == 0, an index out of range or a NULL required
 * pointer.  One stream: k_commit / k_share_eval with D = S, then per chunk of seats e1 = g r on the shared
 * comb, K = pk r (below), the item-indexed encode and k_sym_xor.  The chunk keeps the hybrid stage's
 * scratch within 2 GiB; dkg_ctx_set_batch_full_chunk forces it, counted in SEATS here; outputs do not
 * depend on it.  Phase times (dkg_ctx_phase_ms; summed over the chunks): "seats.commit",
 * "seats.deal_e1", "seats.deal_mul", "seats.deal_encode", "seats.deal_sym"; a phase that did not run
 * reads -1.  Host pointers only: there is no device-pointer variant and no shard form. */
int dkg_party_round1_seats(dkg_ctx *ctx, size_t B, size_t n, size_t t, size_t S, const uint32_t *cer,
                           const uint32_t *js, const uint8_t *a, const uint8_t *b, const uint8_t *r,
                           const uint8_t *pk, uint8_t *E, uint8_t *A, uint8_t *e1, uint8_t *ct, uint8_t *s_out,
                           uint8_t *sp_out, uint8_t *own);
/* How dkg_party_round1_seats computes K = pk_q r (elgamal.rs:138-140).  A dealing seat uses each recipient
 * key for exactly two items, so: 2 = the joint chain (k_seat_enc_mul): one lane per (seat, recipient)
 * walks the signed radix-4 digits of both scalars right to left over M = 4^w pk -- 2 doublings and 2
 * complete additions per window, no table; 1 = a signed radix-16 comb per key slot, k_benc_tab and
 * k_benc_mul with one dealer row per key as the batches run them (80 KiB per slot, in chunks): the
 * yardstick and an independent cross-check; 0 (default) = automatic, by profiles/seat_deal_time.json.
 * Outputs do not depend on it.  dkg_ctx_set_field_mode does not apply to either.  DKG_E_ARG for any other
 * mode. */
int dkg_ctx_set_seat_deal(dkg_ctx *ctx, int mode);
/* The route (1 or 2) the last dkg_party_round1_seats ran; 0 before the first. */
int dkg_ctx_last_seat_deal(const dkg_ctx *ctx);
/* The joint chain's recoding of one scalar, exactly as k_seat_enc_mul computes it (one routine serves
 * both): signed radix-4 digits, sum_w digits[w] 4^w = k, *windows = 128 always; digits[w] in
 * {-2, -1, 0, 1} below the top window, which keeps its value plus the carry in {0, 1, 2} ({0, 1} for
 * k < 2^254, every canonical scalar among them).  DKG_E_ARG for k >= 2^255 or a NULL pointer.  Host-only,
 * a pure function. */
int dkg_seat_enc_digits(const uint8_t k[32], int8_t digits[128], int *windows);

/* ---- hosted seats through rounds 3-5 (seat_finalise.hip) ----
 * What an operator's seats do after their share checks, without one call per ceremony and without data
 * an operator never holds (the n x n share matrix, the other parties' keys).  All calls take B ceremonies
 * of one (n, t) with rows laid out as above (row c * n + i = dealer i of ceremony c) and seats as above.
 * S == 0 (the complaint calls: B == 0) returns DKG_OK and touches nothing; a count of 0 allows NULL list
 * arrays; an index outside its range or a missing required pointer is DKG_E_ARG.
 *
 * Phases<Phase2>::compute_qualified_set (committee.rs:370-398, broadcast.rs:50-99) for the broadcast
 * complaints of MANY ceremonies: flat arrays as dkg_ceremony_batch_verify_full_proven takes them
 * (ceremony[c] 0-based < B, accuser / accused 1-based; ceremonies interleaved, duplicates allowed; verdicts
 * in input order), but enc [C][128] comes from the caller as in dkg_complaints_verify -- no ceremony is
 * replayed.  pk [B][n][32], E [B*n][t+1][32], fetched1 [B*n] (NULL = all present).  verdict [C] and
 * qualified [B][n] (may be NULL) equal what dkg_complaints_verify returns for ceremony g on g's slices and
 * g's own complaints in their relative order: DKG_COMPLAINT_IGNORED, -1, 1, 2, 0 in its precedence.  A
 * ceremony without a complaint is qualified except for missing or undecodable rows.  Only the DISTINCT
 * accused rows of E are uploaded and decoded for the checks; the other rows are decoded (for the "row
 * decodes" term) only when qualified is requested.  The launch count of the checks does not depend on
 * B, and P_i(j) is always one Horner walk per complaint: dkg_ctx_set_complaint_eval does not apply.
 * Requires dkg_env_init (h). */
int dkg_complaints_verify_ceremonies(dkg_ctx *ctx, size_t B, size_t n, size_t t, size_t C, const uint32_t *ceremony,
                                     const uint32_t *accuser, const uint32_t *accused, const uint8_t *pk,
                                     const uint8_t *E, const uint8_t *fetched1, const uint8_t *enc,
                                     const uint8_t *proofs, int32_t *verdict, uint8_t *qualified);
/* Phases<Phase4>::proceed's loop (committee.rs:636-670, broadcast.rs:104-144) for the round-4 complaints of
 * many ceremonies, the same flat arrays; share, randomness [C][32]; E, A [B*n][t+1][32]; qualified,
 * fetched3 [B*n] (NULL = all 1).  verdict [C] and reconstruct [B][n] (may be NULL; all 0 for a ceremony
 * without a complaint) equal dkg_complaints3_verify's for ceremony g: DKG_COMPLAINT_IGNORED,
 * DKG_COMPLAINT_NO_PHASE3, -1, 3, 2, 0 in its precedence.  Only the distinct accused rows of E and A are
 * uploaded and decoded; always the per-complaint Horner walk (dkg_ctx_set_complaint_eval does not
 * apply).  Requires dkg_env_init (h). */
int dkg_complaints3_verify_ceremonies(dkg_ctx *ctx, size_t B, size_t n, size_t t, size_t C, const uint32_t *ceremony,
                                      const uint32_t *accuser, const uint32_t *accused, const uint8_t *share,
                                      const uint8_t *randomness, const uint8_t *E, const uint8_t *A,
                                      const uint8_t *qualified, const uint8_t *fetched3, int32_t *verdict,
                                      uint8_t *reconstruct);
/* Phases<Phase2>::proceed per seat (committee.rs:453-467): qualified [B][n] the round-2 qualified sets,
 * s [S][n][32] the shares addressed to seat p (read reduced mod l, as everywhere).  final_share[p] = the
 * sum over the dealers i with qualified[cer[p]][i] of s[p][i], the seat's own dealer row included as in
 * the reference; public_share[p] (may be NULL) = g final_share[p].  [S][32] each.  The reference's guard
 * at :443 compares qualified_set.len(), which is always n, so it cannot fire under dkg_env_check: there is
 * no error output.  One launch set for all seats.  Needs no dkg_env_init. */
int dkg_party_round3_seats(dkg_ctx *ctx, size_t B, size_t n, size_t t, size_t S, const uint32_t *cer,
                           const uint32_t *js, const uint8_t *qualified, const uint8_t *s, uint8_t *final_share,
                           uint8_t *public_share);
/* Phases<Phase5>::finalise per seat (committee.rs:726-805).  qualified, reconstruct [B][n]; fetched3 [B*n]
 * (NULL = all present); r2_error, r4_error [S] (NULL = none): the SEAT's own Phase1 / Phase3 outcomes;
 * A0 [B*n][32] the dealers' A_i0; s [S][n][32] the seat's own column.  The D5 disclosures are the flat
 * form of the BroadcastPhase5 messages the operator fetched (a Vec<Option<share>> per dealer, so a sender
 * may disclose for some dealers only): entry d = sender d_sender[d] of ceremony d_ceremony[d] disclosed
 * dealer d_dealer[d]'s share d_share[d] (sender, dealer 1-based; shares read reduced mod l).
 * Seat p: R2_ERROR, R4_ERROR, then PHASE4_ERROR (qualified - reconstruct <= t in its ceremony, :673-677);
 * then the dealers in index order, the first failure wins (:745-797).  A reconstructed dealer i is
 * interpolated at zero through the seat's own (js[p] + 1, s[p][i]) and every listed disclosure for (its
 * ceremony, i) by a sender q != js[p] + 1 that is a final party (qualified and not reconstructed, :765);
 * fewer than t points: DKG_FIN_INSUFFICIENT with index i (exactly t interpolate, as the reference).  A
 * dealer that is not reconstructed adds A0[i] if it is qualified or the seat itself; DKG_FIN_PANIC with
 * index i if it is disqualified and not the seat, and also if it is qualified but fetched3[i] == 0 or its
 * A0 does not decode (the rule of dkg_ceremony_verify_fetched_proven, not a whole-call DKG_E_DECODE).
 * mpk[p] = the sum of those A0 + g (the sum of the recovered secrets), 32 zero bytes unless status[p] ==
 * DKG_FIN_OK; recovery_index[p] (may be NULL) = -1 unless INSUFFICIENT or PANIC.
 * Entries the reference's loop never reads are ignored: a sender that is not a final party, a dealer that
 * is not reconstructed, the seat's own sender.  A ceremony no seat names is never interpreted.
 * DKG_E_ARG: a duplicate (ceremony, sender, dealer), an index outside its range, reconstruct without
 * qualified in a named ceremony (:746-747 panics).  DKG_E_DECODE only for the own A0 of a disqualified
 * seat that finalises.  The status of every seat is dkg_seat_finalise_status's.  One 64-lane workgroup
 * per seat interpolates (k_seat_lagrange); host work O(S n + D5).  Phase times "seats.lagrange" and
 * "seats.mpk" (one stream).  Needs no dkg_env_init. */
int dkg_finalise_seats(dkg_ctx *ctx, size_t B, size_t n, size_t t, size_t S, const uint32_t *cer, const uint32_t *js,
                       const uint8_t *qualified, const uint8_t *reconstruct, const uint8_t *fetched3,
                       const uint8_t *r2_error, const uint8_t *r4_error, const uint8_t *A0, const uint8_t *s,
                       size_t D5, const uint32_t *d_ceremony, const uint32_t *d_sender, const uint32_t *d_dealer,
                       const uint8_t *d_share, uint8_t *mpk, int32_t *status, int32_t *recovery_index);
/* The status rule of dkg_finalise_seats for ONE seat p (0-based) as a pure host function (no GPU, no
 * context): qualified, reconstruct [n]; a_present [n] (NULL = all): dealer i's A_i0 was fetched and
 * decodes; points [n]: the points the seat holds for dealer i (its own included; read for reconstructed
 * dealers only); r2_error, r4_error the seat's own.  Returns the DKG_FIN_* code, *recovery_index (may be
 * NULL) as above; DKG_E_ARG for n == 0, p >= n, a NULL required pointer or reconstruct without qualified. */
int dkg_seat_finalise_status(size_t n, size_t t, size_t p, const uint8_t *qualified, const uint8_t *reconstruct,
                             const uint8_t *a_present, const uint32_t *points, int r2_error, int r4_error,
                             int32_t *recovery_index);

/* ---- public shares of every party from the broadcast commitments (pubshares.hip) ----
 * The verification keys g s_j of a finished ceremony from PUBLIC data alone.  s_j is the sum over the final
 * dealers of s_ij (committee.rs:453-461), and round 4 accepted g s_ij = sum_k (j+1)^k A_i[k] for every dealer
 * that stays (:532-539), so with S[k] = the sum over those dealers of A_i[k]
 *   public_share[j] = sum_k (j+1)^k S[k]  +  g (the sum over the reconstructed dealers i of s_ij).
 * A reconstructed dealer's A_i is missing or proven inconsistent; its term is the share party j itself
 * disclosed in phase 5 (BroadcastPhase5, committee.rs:660-669), which is public: no interpolation.
 * The value equals g final_share_j (what the drivers and dkg_party_round3_seats compute from the secret share,
 * :462-467) for a party whose checks accepted every dealer used.  The master public key stays with the
 * finalise calls: S[0] lacks the reconstructed dealers' secrets (:784-789).
 * Rows as in the batch and seats calls: A [B*n][t+1][32], row c * n + i = dealer i of ceremony c. */
#define DKG_PS_OK 0
#define DKG_PS_NO_COMMITMENT 1 /* a dealer the sum uses was not fetched or does not decode */
#define DKG_PS_NO_DISCLOSURE 2 /* index j disclosed no share of some reconstructed dealer */
/* S[c][k] = the sum over the dealers i with mask[c][i] of A_{c,i}[k], compressed: the aggregated committed
 * polynomial of MembersFetchedState3's vectors (committee.rs:520-559 reads them one dealer at a time).  mask
 * [B][n] (NULL = all dealers); S [B][t+1][32]; ok[c] (may be NULL) = 0, and row c of S zero bytes, where a masked
 * row does not decode -- a row outside the mask is never interpreted.  An empty mask gives the identity in every
 * coefficient: 32 zero bytes with ok = 1.  B == 0 returns DKG_OK and touches nothing; DKG_E_ARG for n == 0, a
 * NULL A or S, or more than 2^32 - 1 rows.  One 64-lane workgroup per column (c, k) adds the dealers with the
 * complete formula (k_commit_colsum); the rows are uploaded and decoded in slabs (below).  Phase times (one
 * stream): "pubshares.decode", "pubshares.sum".  Needs no dkg_env_init. */
int dkg_commitment_sum(dkg_ctx *ctx, size_t B, size_t n, size_t t, const uint8_t *A, const uint8_t *mask, uint8_t *S,
                       uint8_t *ok);
/* V[c][m] = the public share of party js[m] of ceremony c, [B][M][32] (the layout of the batch drivers'
 * public_share): sum_k (js[m]+1)^k S_c[k] + g (the sum over the dealers i reconstructed in c of
 * d_share(c, js[m]+1, i+1)).  Dealer i of ceremony c enters S_c iff qualified[c][i] && !reconstruct[c][i]
 * (:733-739); qualified [B][n]; reconstruct [B][n] (NULL = none; reconstruct without qualified is DKG_E_ARG,
 * :746-747 panics); fetched3 [B*n] (NULL = all present).  js [M]: 0-based, below n (DKG_E_ARG otherwise), any
 * order, repeats allowed, one list for all ceremonies.  The D5 disclosures are dkg_finalise_seats' flat form
 * (sender, dealer 1-based; shares read reduced mod l); a duplicate (ceremony, sender, dealer) or an index out of
 * range is DKG_E_ARG; entries of dealers that are not reconstructed, or of senders not in js, are ignored.
 * status [B][M] and which [B][M] (may be NULL) are exactly dkg_public_share_status's for the ceremony's slices,
 * a_present = fetched and decodes.  V is 32 zero bytes unless the status is DKG_PS_OK -- the identity encodes as
 * zero bytes too, so read the status.  S (may be NULL) = dkg_commitment_sum's output for the call's mask.
 * B == 0 or M == 0 returns DKG_OK and touches nothing.  S_c is evaluated by dkg_commitment_eval's evaluator
 * with the B ceremonies as its rows and js as its indices: dkg_ctx_set_receiver_chunk and
 * dkg_ctx_set_field_mode apply as they do there; outputs do not depend on them.  g's comb is built in
 * dkg_ctx_create: needs no dkg_env_init.  Phase times (one stream): "pubshares.decode", "pubshares.sum",
 * "pubshares.eval", "pubshares.disclosed" (-1 when no disclosure is used).  Host pointers, one device. */
int dkg_public_shares(dkg_ctx *ctx, size_t B, size_t n, size_t t, const uint8_t *A, const uint8_t *qualified,
                      const uint8_t *reconstruct, const uint8_t *fetched3, size_t M, const uint32_t *js, size_t D5,
                      const uint32_t *d_ceremony, const uint32_t *d_sender, const uint32_t *d_dealer,
                      const uint8_t *d_share, uint8_t *V, int32_t *status, int32_t *which, uint8_t *S);
/* The status of dkg_public_shares for ONE ceremony and one 0-based index j, a pure host function (no GPU, no
 * context): qualified [n]; reconstruct [n] (NULL = none); a_present [n] (NULL = all): dealer i's round-3 vector
 * was fetched and decodes (committee.rs:527-530 stores nothing otherwise); the D5 disclosures (sender, dealer)
 * of that ceremony, 1-based.  DKG_PS_NO_COMMITMENT wins, *which (may be NULL) the lowest 0-based dealer that
 * is used (qualified, not reconstructed) but absent; otherwise DKG_PS_NO_DISCLOSURE with the lowest
 * reconstructed dealer i without an entry (j + 1, i + 1) (:660-669); otherwise DKG_PS_OK and -1.  DKG_E_ARG
 * for n == 0, j >= n, a NULL qualified (or a NULL list with D5 > 0), reconstruct without qualified, an index
 * outside 1..n, or a duplicate pair. */
int dkg_public_share_status(size_t n, const uint8_t *qualified, const uint8_t *reconstruct, const uint8_t *a_present,
                            uint32_t j, size_t D5, const uint32_t *d_sender, const uint32_t *d_dealer,
                            int32_t *which);
/* Rows of A that dkg_commitment_sum / dkg_public_shares upload and decode at a time: 0 (default) = automatic,
 * as many as 256 MiB of decoded points hold; >= 1 forced (a slab may cut through a ceremony).  Outputs do not
 * depend on it.  DKG_E_ARG for more than 2^30 rows. */
int dkg_ctx_set_public_share_slab(dkg_ctx *ctx, size_t rows);

/* ---- whole ceremony (rounds 1-5, every party played in one process as the reference tests do,
 * committee.rs:1518-1656) in plaintext-share mode. ---- */
typedef struct {
  /* host outputs; any pointer may be NULL */
  uint8_t *E, *A;               /* [n][t+1][32] (round-1 broadcast; A = round-3 broadcast) */
  uint8_t *s, *s_prime;         /* [n][n][32] */
  uint8_t *dec2, *dec4;         /* [n dealer][n receiver] */
  uint8_t *qualified;           /* [n] common qualified set after round 3 */
  uint8_t *r2_error;            /* [n] receiver j: more than t complaints (MisbehaviourHigherThreshold) */
  uint8_t *r4_error;            /* [n] receiver j: fewer than t+1 honest dealers (itself included) in
                                   round 4, MisbehaviourHigherThreshold (committee.rs:567-569) */
  int32_t *complaints2;         /* [n] complaints raised by receiver j in round 2 */
  uint8_t *reconstruct;         /* [n] dealers whose secret is reconstructed in finalise */
  uint8_t *final_share;         /* [n][32] s_j = sum_{i in Q} s_ij (committee.rs:454-462) */
  uint8_t *public_share;        /* [n][32] g * s_j (committee.rs:464-466) */
  uint8_t mpk[32];              /* MasterPublicKey (committee.rs:726-805) that every finalising
                                   final party (qualified, not reconstructable, no r2 / r4 error)
                                   computes when all phase-5 disclosures arrive: a reconstructed
                                   dealer's secret is interpolated at zero over exactly the shares of
                                   the final parties that disclose (:754-788) -- a party with an r2 /
                                   r4 error never broadcasts its phase-5 shares (:340-347, 567-569,
                                   684); with exactly t of them a wrong secret, as the reference.
                                   ALL ZERO and meaningless when phase4_error == 1, and when a
                                   dealer is reconstructed and fewer than t final parties disclose
                                   (InsufficientSharesForRecovery for everyone, :779-781).
                                   Other parties' views, and missing disclosures:
                                   dkg_finalise_parties. */
  int32_t n_qualified;
  int32_t phase4_error;         /* 1: qualified minus reconstructable <= t, every party's
                                   Phases<Phase4>::proceed fails with MisbehaviourHigherThreshold
                                   (committee.rs:673-677): nobody finalises, there is no mpk */
  /* device times of each phase, milliseconds (HIP events) */
  double ms_round1, ms_round2, ms_round3, ms_round4, ms_finalise, ms_total;
} dkg_ceremony_out;

/* Honest run from coefficients a, b ([n][t+1][32], host). */
int dkg_ceremony_run(dkg_ctx *ctx, size_t n, size_t t, const uint8_t *a, const uint8_t *b, dkg_ceremony_out *out);
/* Receiver side (rounds 2-5) from broadcast values that may have been tampered with:
 * E, A [n][t+1][32]; s, s_prime [n][n][32]; all four required (DKG_E_ARG when NULL), here and in
 * dkg_ceremony_verify_fetched. */
int dkg_ceremony_verify(dkg_ctx *ctx, size_t n, size_t t, const uint8_t *E, const uint8_t *A, const uint8_t *s,
                        const uint8_t *s_prime, dkg_ceremony_out *out);
/* dkg_ceremony_verify after the broadcast intake of MembersFetchedState1/3::from_broadcast
 * (committee.rs:825-870, 921-966): fetched1[i] = 0 when dealer i's phase-1 broadcast is absent or
 * malformed (committed_coefficients.len() != t+1 or encrypted_shares.len() != n): no fetched data,
 * DKG_MISSING for every receiver in round 2 (disqualified, no complaint, :331-335).
 * fetched3[i] = 0 when its phase-3 broadcast is absent or has the wrong length: a qualified dealer
 * is accused by every receiver in round 4 (:549-555) and reconstructed.  The E / A rows of such
 * dealers are not read for decisions (any bytes). */
int dkg_ceremony_verify_fetched(dkg_ctx *ctx, size_t n, size_t t, const uint8_t *E, const uint8_t *A,
                                const uint8_t *s, const uint8_t *s_prime, const uint8_t *fetched1,
                                const uint8_t *fetched3, dkg_ceremony_out *out);
/* Device-resident variant for benchmarks: d_a, d_b are device pointers to [n][t+1][32] canonical
 * scalars; intermediates stay in HBM; only the small outputs (mpk, flags, counts, timings) are
 * copied back into *out (its array pointers are ignored except qualified / r2_error / r4_error / complaints2). */
int dkg_ceremony_run_device(dkg_ctx *ctx, size_t n, size_t t, const void *d_a, const void *d_b,
                            dkg_ceremony_out *out);
/* Sharded variant (one rank of a multi-GPU run): this ctx owns dealers [d0, d1) of the same
 * ceremony.  Produces this rank's commitments E/A and decision rows; the caller all-gathers
 * (RCCL over xGMI) the rows, A_0 values and share partial sums.  Device pointers throughout:
 * d_a, d_b [d1-d0][t+1][32]; d_dec2, d_dec4 [d1-d0][n]; d_A0 [d1-d0][32] = each dealer's
 * compressed master-key term A_i0 (a dealer that round-4 accusations put in the reconstructable set
 * gets g * a_i0 after the exchange, dkg_ceremony_shard_recon_device, because the interpolation
 * points -- the final parties -- depend on every rank's rows; then mpk = sum of the qualified
 * dealers' terms); d_partial [n][32] = sum over this rank's QUALIFIED dealers of s_ij (qualification
 * of a dealer is decided by its own round-2 row, so it needs no exchange).
 * Arguments, here and in the five dkg_ceremony_shard_*_device calls below: d_partial (written even for a
 * rank without dealers, d0 == d1) and the host keys a call takes are always required; with d0 < d1 so are
 * its device inputs and d_dec2, d_dec4, d_A0.  A null one is DKG_E_ARG, before anything is queued. */
int dkg_ceremony_shard_device(dkg_ctx *ctx, size_t n, size_t t, size_t d0, size_t d1, const void *d_a,
                              const void *d_b, void *d_dec2, void *d_dec4, void *d_A0, void *d_partial,
                              double *ms_total);
/* Sharded verification of received broadcasts (the rank's dealers' rows of MembersFetchedState1 /
 * Phase1 / Phase3, committee.rs:260-366, 508-580, 726-805): d_E, d_A [d1-d0][t+1][32] compressed
 * commitments as broadcast, d_s, d_s_prime [d1-d0][n][32] the shares (Scalar::from_bytes
 * semantics).  Outputs as dkg_ceremony_shard_device; an undecodable E row is DKG_MISSING in round 2
 * (disqualified, no complaint), an undecodable A row an accusation in round 4. */
int dkg_ceremony_shard_verify_device(dkg_ctx *ctx, size_t n, size_t t, size_t d0, size_t d1, const void *d_E,
                                     const void *d_A, const void *d_s, const void *d_s_prime, void *d_dec2,
                                     void *d_dec4, void *d_A0, void *d_partial, double *ms_total);
/* Full (encrypted-share) mode of the sharded variant: what dkg_ceremony_run_full_device does, on this
 * rank's dealers [d0, d1) -- round 1 for the D = d1 - d0 dealers, their shares hybrid-encrypted to all
 * n sorted member keys (committee.rs:164-172; elgamal.rs:134-193), all n receivers' decryption of those
 * rows (committee.rs:282-286), and the round-2/4 checks on the DECRYPTED shares.  d_a, d_b as
 * dkg_ceremony_shard_device; d_r device [D][n][2][32] canonical encryption randomness (what
 * dkg_enc_randomness_device(.., d0, D, ..) writes); sk, pk host [n][32] (dkg_member_keys); d_e1, d_ct
 * device [D][n][2][32] (either may be NULL) receive this rank's round-1 ciphertext broadcast.  Outputs
 * as dkg_ceremony_shard_device; the decrypted shares become the rows dkg_ceremony_shard_recon_device
 * reads with d_s = NULL.  Which comb serves K = pk_q r: dkg_ctx_set_key_comb. */
int dkg_ceremony_shard_full_device(dkg_ctx *ctx, size_t n, size_t t, size_t d0, size_t d1, const void *d_a,
                                   const void *d_b, const void *d_r, const uint8_t *sk, const uint8_t *pk, void *d_e1,
                                   void *d_ct, void *d_dec2, void *d_dec4, void *d_A0, void *d_partial,
                                   double *ms_total);
/* Full mode of dkg_ceremony_shard_verify_device (what dkg_ceremony_verify_full does, on rows [d0, d1)):
 * d_e1, d_ct device [D][n][2][32] the rank's dealers' (possibly tampered) ciphertexts, sk host [n][32].
 * A dealer with any item whose e1 does not decode is missing data: a DKG_MISSING row in round 2, like
 * an undecodable E row.  The decrypted shares become the ctx's remembered shard rows. */
int dkg_ceremony_shard_verify_full_device(dkg_ctx *ctx, size_t n, size_t t, size_t d0, size_t d1, const void *d_E,
                                          const void *d_A, const void *d_e1, const void *d_ct, const uint8_t *sk,
                                          void *d_dec2, void *d_dec4, void *d_A0, void *d_partial, double *ms_total);
/* Which comb of the recipient keys serves full mode's K = pk_q r (elgamal.rs:138-140) wherever the
 * single-ceremony encryption runs (dkg_encrypt_shares, dkg_ceremony_run_full_device, the sharded full
 * calls): 1 = radix 2^DKG_KEY_COMB_BITS tables (1.7 MB per key at 2^10, one mixed addition per window),
 * 2 = signed radix-16 combs (80 KiB per key, 64 complete additions; the batches' tables).  0 (default):
 * dkg_encrypt_shares and dkg_ceremony_run_full_device use kind 1, as they always have, and the sharded
 * full calls choose by dkg_key_comb_choice.  Both kinds are cached by the keys' bytes, separately.
 * Outputs do not depend on it.  DKG_E_ARG for any other mode. */
int dkg_ctx_set_key_comb(dkg_ctx *ctx, int mode);
/* The kind (1 or 2) of the last single-ceremony encryption on this ctx; 0 before the first. */
int dkg_ctx_last_key_comb(const dkg_ctx *ctx);
/* The cost rule behind mode 0 of the sharded full calls (a host function, no ctx): the kind with the
 * smaller (cached ? 0 : build(keys)) + mul_per_item * keys * items_per_key; items_per_key = 2 D for a
 * shard of D dealers.  A tie keeps kind 1. */
int dkg_key_comb_choice(size_t keys, size_t items_per_key, int cached10, int cached16);
/* The rule's constants, build(keys) = floor + per key * keys: c[0] the radix-2^BITS build's floor, us;
 * c[1] that build, us per key; c[2] its multiplication, ns per item; c[3], c[4], c[5] the same for
 * radix 16.  Measured: profiles/shard_full_time.json. */
void dkg_key_comb_constants(double c[6]);
/* Finalise step of a sharded run, after the exchange (committee.rs:747-789): for this rank's dealers
 * [d0, d1) with reconstruct[i] (host [n], the combined round-4 outcome), d_terms[i - d0] (device
 * [d1-d0][32], the rank's exchanged master-key terms, in/out) is replaced by g * a_i0 recovered by
 * Lagrange interpolation at zero over the shares of the DISCLOSING final parties: qualified[j] &&
 * !reconstruct[j] && !r2_error[j] && !r4_error[j] (host [n]; r2_error / r4_error may be NULL) -- a
 * party whose Phase1 or Phase3 failed never broadcasts its phase-5 disclosures (:340-347, 567-569,
 * 684) -- the value every finalising party computes.  When some dealer is reconstructed and fewer
 * than t parties disclose, every finalising party fails with InsufficientSharesForRecovery
 * (:779-781): *recovery_error (may be NULL) = 1, d_terms is untouched and the caller has no mpk
 * (pass it as phase4_error to dkg_shard_finalise_device); else 0.  It depends on the common outcome
 * only, so every rank gets the same.  d_s: the dealers' share rows [d1-d0][n][32] (from_bits
 * semantics), or NULL for the rows of the last dkg_ceremony_shard_device / _shard_verify_device call
 * on this ctx (same n, d0, d1).  Dealers without reconstruct are untouched. */
int dkg_ceremony_shard_recon_device(dkg_ctx *ctx, size_t n, size_t t, size_t d0, size_t d1, const uint8_t *qualified,
                                    const uint8_t *reconstruct, const uint8_t *r2_error, const uint8_t *r4_error,
                                    const void *d_s, void *d_terms, int32_t *recovery_error);
/* Combine step of the sharded run (device pointers):
 * round-3 sum (committee.rs:454-462): out[j] = sum over rows r with mask[r] (NULL = all) of in[r][j]
 * mod l; in [rows][n][32] canonical scalars (e.g. the all-gathered per-rank partials), out [n][32]. */
int dkg_scalar_sum_device(dkg_ctx *ctx, size_t rows, size_t n, const void *d_in, const void *d_mask, void *d_out);
/* finalise (committee.rs:790-795): out = sum of points[c] with mask[c] (NULL = all), points
 * [count][32] compressed, out [32] compressed.  DKG_E_DECODE if a selected point does not decode. */
int dkg_point_sum_device(dkg_ctx *ctx, size_t count, const void *d_points, const void *d_mask, void *d_out);

/* ---- the sharded run's protocol layer (multi-GPU, one process per GPU) ----
 * The reference has no transport (its broadcast channel is abstract, src/lib.rs:91-115); a
 * multi-rank driver supplies the all-gathers (RCCL over xGMI) and calls, on every rank:
 *   dkg_ceremony_shard_device / _shard_verify_device   this rank's dealers' rows
 *   all-gather dec2, dec4 (each rank's [R][n] block), A0 ([R][32]), partials ([n][32])
 *   dkg_shard_combine_device                           the common outcome (identical on every rank)
 *   if reconstruct has any member and !phase4_error:
 *     dkg_ceremony_shard_recon_device, all-gather the terms again (unless recovery_error)
 *   dkg_shard_finalise_device                          final shares, public shares, mpk
 * Rank r of world_size owns dealers [r*n/ws, (r+1)*n/ws); R = dkg_shard_rows(n, ws) is the padded
 * block height every rank gathers. */
void dkg_shard_range(size_t n, size_t world_size, size_t rank, size_t *d0, size_t *d1);
size_t dkg_shard_rows(size_t n, size_t world_size);

typedef struct {
  /* host arrays [n] (any may be NULL) */
  uint8_t *qualified;     /* round 2: no REJECT and no MISSING in the dealer's row (committee.rs:311-335, 370-398) */
  int32_t *complaints2;   /* REJECTs raised by receiver j */
  uint8_t *r2_error;      /* complaints2[j] > t (:340-347) */
  uint8_t *reconstruct;   /* qualified dealers some receiver rejected in round 4 (:660-670) */
  uint8_t *r4_error;      /* receiver j: itself plus the qualified dealers it accepted < t+1 (:515-516, 567-569) */
  int32_t n_qualified;
  int32_t phase4_error;   /* qualified minus reconstructable <= t (:673-677) */
} dkg_shard_outcome;

/* Combine step after the decision all-gathers: d_dec2_g, d_dec4_g device [ws][R][n] (rank blocks as
 * gathered, rows past a rank's dealer count ignored).  Derives the common outcome with the same code
 * as the single-GPU drivers (runtime.hip round2_device / round4_device and their host halves).  d_dec2, d_dec4 (device
 * [n][n], may be NULL): the compacted decision matrices, dec4 with the SKIPPED rows of disqualified
 * dealers applied (:522). */
int dkg_shard_combine_device(dkg_ctx *ctx, size_t n, size_t t, size_t world_size, const void *d_dec2_g,
                             const void *d_dec4_g, void *d_dec2, void *d_dec4, dkg_shard_outcome *out);
/* Packed decision rows: the complaint / verification bitmaps a multi-rank driver all-gathers instead
 * of n bytes per row (committee.rs:311-347: every party learns every complaint).  A rank's raw rows
 * hold REJECT / ACCEPT (round 4 too: SKIPPED is applied by the combine), SELF on the global diagonal
 * and, in round 2, whole rows of MISSING; row r becomes dkg_packed_row_words(n) = ceil(n/32) + 1
 * little-endian u32 words: bit j % 32 of word j / 32 set iff entry j is ACCEPT, then a kind word (0
 * checked, 1 MISSING row, 2 SKIPPED row).  n = 4096: 516 bytes per row instead of 4096. */
size_t dkg_packed_row_words(size_t n);
/* Windows (one mixed addition each) per scalar of the fixed-base combs of g and h the checks and
 * commitments use (radix 2^DKG_COMBW_BITS, a build-time choice): the closed-form work of bench.py. */
int dkg_fixed_base_windows(void);
/* The same for the member keys' combs (full mode's K = pk_q r, radix 2^DKG_KEY_COMB_BITS). */
int dkg_key_comb_windows(void);
/* How the radix-2^BITS comb tables are built (the g and h combs of dkg_ctx_create / dkg_env_init, a
 * caller base's comb in dkg_fixed_base_batch, the member keys' radix-2^DKG_KEY_COMB_BITS combs of full
 * mode): 1 = one thread per entry (its own doublings, multiple and inversion), 2 = chained (one
 * doubling chain per base for the windows' bases, then each thread walks a chunk of consecutive
 * entries by mixed additions and inverts the chunk's Z together), 0 (default) = automatic: chained for
 * both radices (DESIGN.md section 4 has the measured ratios).  Governs every comb built after the call
 * and drops the cached caller-base comb and the cached member-key combs, so their next use rebuilds
 * them.  The generator's comb of dkg_ctx_create is built under automatic.  The tables' canonical
 * contents (dkg_comb_entries) and every output computed from them do not depend on the builder.
 * DKG_E_ARG for any other mode. */
int dkg_ctx_set_comb_build(dkg_ctx *ctx, int mode);
/* The builder (1 or 2) the last comb build on this ctx ran; 0 before the first. */
int dkg_ctx_last_comb_build(const dkg_ctx *ctx);
/* Device time of that build in ms (events around its launches; waits for it to finish). */
double dkg_ctx_last_comb_build_ms(const dkg_ctx *ctx);
/* The geometry of a comb kind (a host function, no ctx, no GPU): kind 0 = the shared bases' comb
 * (radix 2^DKG_COMBW_BITS), kind 1 = the member keys' comb (radix 2^DKG_KEY_COMB_BITS).  *bits the
 * radix' exponent, *windows = 256 / bits + 1, *entries = 2^(bits - 1) per window, *chunk the
 * consecutive entries one thread of the chained builder owns.  Outputs may be NULL.  DKG_E_ARG for
 * any other kind. */
int dkg_comb_geometry(int kind, int *bits, int *windows, uint32_t *entries, uint32_t *chunk);
/* Builds the comb of `base` (32-byte encoding; NULL = the generator) with the ctx's current builder --
 * always a fresh build: no cached table is read and none is kept (a kind-0 build takes the caller
 * base's buffer of dkg_fixed_base_batch, whose cached comb is dropped) -- and writes entries
 * d = first + 1 .. first + count of `window`, entry d = d * 2^(bits * window) * base, as out
 * [count][96]: the canonical little-endian encodings of y + x, y - x and 2 d_curve x y of the affine
 * point.  DKG_E_DECODE for a base that does not decode, DKG_E_ARG for a kind, window or range outside
 * the geometry; count == 0 returns DKG_OK and touches nothing. */
int dkg_comb_entries(dkg_ctx *ctx, int kind, const uint8_t base[32], int window, uint32_t first, uint32_t count,
                     uint8_t *out);
/* d_dec device [nvalid][n] raw rows of dealers d0 .. d0+nvalid-1 (dkg_ceremony_shard_device's
 * output) -> d_packed device [rows][dkg_packed_row_words(n)] u32, rows past nvalid zero (the padded
 * rank block, rows = dkg_shard_rows).  DKG_E_ARG if a row holds values the encoding cannot carry
 * (nothing is lost silently). */
int dkg_decisions_pack_device(dkg_ctx *ctx, size_t rows, size_t nvalid, size_t n, size_t d0, const void *d_dec,
                              void *d_packed);
/* dkg_shard_combine_device on the gathered packed blocks: d_pack2_g, d_pack4_g device
 * [ws][R][dkg_packed_row_words(n)] u32; outputs as dkg_shard_combine_device (d_dec2 / d_dec4 are the
 * unpacked matrices, bit-identical to the byte exchange's). */
int dkg_shard_combine_packed_device(dkg_ctx *ctx, size_t n, size_t t, size_t world_size, const void *d_pack2_g,
                                    const void *d_pack4_g, void *d_dec2, void *d_dec4, dkg_shard_outcome *out);
/* Finalise of the sharded run: d_terms_g device [ws][R][32] the gathered master-key terms (A_i0, or
 * g * a_i0 for reconstructed dealers after dkg_ceremony_shard_recon_device), d_partials_g device
 * [ws][n][32] the gathered partial final shares, qualified host [n] (the combine's).  Outputs:
 * d_final_share device [n][32] s_j = sum of the partials (committee.rs:454-462), d_public_share device
 * [n][32] g * s_j (:463-467; may be NULL), mpk host [32] = sum of the qualified dealers' terms
 * (:790-795), zero when phase4_error (nobody finalises, :673-677). */
int dkg_shard_finalise_device(dkg_ctx *ctx, size_t n, size_t t, size_t world_size, const void *d_terms_g,
                              const void *d_partials_g, const uint8_t *qualified, int phase4_error,
                              void *d_final_share, void *d_public_share, uint8_t *mpk);

/* ---- in-library multi-device context: ONE process, several GPUs (SURVEY.md section 8(b),
 * threading row; dkg_amd/csrc/multi.cpp) ----
 * The same dealer sharding as the one-process-per-GPU protocol above, driven inside the library:
 * shard i (on devices[i]) owns dealers dkg_shard_range(n, ndev, i) and runs them on its own host
 * thread; the exchange is a gather of every shard's rows, master-key terms and partial shares into
 * devices[0] by peer copies over xGMI; the combine, the round-4 reconstruction (on the owning
 * shards) and the finalise are the dkg_shard_* steps.  Outputs equal dkg_ceremony_run /
 * dkg_ceremony_verify's.  A device may be listed more than once (its shards share the GPU).
 * The reference is single-threaded and has no transport (src/lib.rs:91-115); this replaces the
 * caller's loop over parties (committee.rs:1518-1656) spread over a node's GPUs.  Not re-entrant
 * on the same context. */
typedef struct dkg_multi dkg_multi;
int dkg_multi_create(const int *devices, int ndev, dkg_multi **out);
void dkg_multi_destroy(dkg_multi *m);
int dkg_multi_size(const dkg_multi *m);
/* shard i's dkg_ctx (its tuning knobs: dkg_ctx_set_split, _set_streams, ...); owned by m */
dkg_ctx *dkg_multi_ctx(dkg_multi *m, int shard);
const char *dkg_multi_last_error(const dkg_multi *m);
/* host wall milliseconds of the last ceremony's steps: "shard_max" / "shard_min" (the shards' device
 * times), "exchange", "combine", "recon", "finalise"; -1 if unknown */
double dkg_multi_phase_ms(const dkg_multi *m, const char *name);
/* Environment::init (committee.rs:72-83) on every shard's context */
int dkg_multi_env_init(dkg_multi *m, size_t threshold, size_t nr_members, const uint8_t *ck_bytes, size_t ck_len,
                       uint8_t h_out[32]);
/* dkg_ceremony_run over the shards: a, b host [n][t+1][32].  out->E, A, s, s_prime must be NULL
 * (they stay on the shards' devices); every other output as dkg_ceremony_run.  Times: ms_round2 =
 * the slowest shard, ms_round3 = exchange, ms_round4 = combine + reconstruction, ms_finalise,
 * ms_total = host wall from the shards' start (after the uploads) to the outputs. */
int dkg_multi_ceremony_run(dkg_multi *m, size_t n, size_t t, const uint8_t *a, const uint8_t *b,
                           dkg_ceremony_out *out);
/* d_a[i], d_b[i]: device pointers on devices[i] to shard i's dealers' coefficients [D_i][t+1][32] */
int dkg_multi_ceremony_run_device(dkg_multi *m, size_t n, size_t t, const void *const *d_a, const void *const *d_b,
                                  dkg_ceremony_out *out);
/* dkg_ceremony_verify over the shards (received broadcasts, host arrays as there) */
int dkg_multi_ceremony_verify(dkg_multi *m, size_t n, size_t t, const uint8_t *E, const uint8_t *A, const uint8_t *s,
                              const uint8_t *s_prime, dkg_ceremony_out *out);
/* Full (encrypted-share) mode over the shards (dkg_ceremony_shard_full_device per shard): a, b host
 * [n][t+1][32], r host [n][n][2][32] (dkg_enc_randomness), sk, pk host [n][32].  out as
 * dkg_multi_ceremony_run (E, A, s, s_prime NULL); the uploads precede the timed region. */
int dkg_multi_ceremony_run_full(dkg_multi *m, size_t n, size_t t, const uint8_t *a, const uint8_t *b,
                                const uint8_t *r, const uint8_t *sk, const uint8_t *pk, dkg_ceremony_out *out);
/* d_a[i], d_b[i] [D_i][t+1][32], d_r[i] [D_i][n][2][32]: device pointers on devices[i] */
int dkg_multi_ceremony_run_full_device(dkg_multi *m, size_t n, size_t t, const void *const *d_a,
                                       const void *const *d_b, const void *const *d_r, const uint8_t *sk,
                                       const uint8_t *pk, dkg_ceremony_out *out);
/* dkg_ceremony_verify_full over the shards (dkg_ceremony_shard_verify_full_device per shard): host
 * arrays as there. */
int dkg_multi_ceremony_verify_full(dkg_multi *m, size_t n, size_t t, const uint8_t *E, const uint8_t *A,
                                   const uint8_t *e1, const uint8_t *ct, const uint8_t *sk, dkg_ceremony_out *out);

/* ---- per-party finalise: Phases<Phase5>::finalise (committee.rs:726-805) as EVERY party p runs it ----
 * Inputs are the ceremony's common outcome (host arrays [n]): qualified, reconstruct (round 4,
 * committee.rs:660-670), r2_error / r4_error (may be NULL: a party whose Phase1 / Phase3 proceed failed
 * never finalises), disclosed (may be NULL = all): 0 for a party whose phase-5 broadcast (its
 * disclosed shares, BroadcastPhase5) party p does not fetch; A0 [n][32] the dealers' A_i0 (phase-3
 * broadcasts); s [n dealer][n receiver][32] the shares.  For each reconstructed dealer i party p
 * interpolates at zero over its own share s_ip and the disclosed shares of the OTHER final parties
 * (:754-775); it fails with InsufficientSharesForRecovery(i) -- i the first reconstructed dealer --
 * when it has fewer than `threshold` = t points (:779-781; exactly t points interpolate a wrong
 * secret, as the reference does).  Outputs [n]: mpk[p] (32 bytes, zero unless status[p] == OK),
 * status[p], recovery_index[p] (the dealer i of InsufficientSharesForRecovery / the panic, else
 * -1; may be NULL).  Dealers are visited in index order and the first failure wins, as in the loop
 * of committee.rs:745-797. */
#define DKG_FIN_OK 0
#define DKG_FIN_R2_ERROR 1      /* Phases<Phase1>::proceed: MisbehaviourHigherThreshold (committee.rs:340-347) */
#define DKG_FIN_R4_ERROR 2      /* Phases<Phase3>::proceed: MisbehaviourHigherThreshold (committee.rs:567-569) */
#define DKG_FIN_PHASE4_ERROR 3  /* Phases<Phase4>::proceed: MisbehaviourHigherThreshold (committee.rs:673-677) */
#define DKG_FIN_INSUFFICIENT 4  /* finalise: InsufficientSharesForRecovery(i) (committee.rs:779-781) */
#define DKG_FIN_PANIC 5         /* finalise panics at dealer i: i is disqualified and i != p, so its
                                   committed coefficients were never recorded (committee.rs:791-794
                                   expect()s them; they are stored only at :190 and :527-530).  A
                                   disqualified party p itself adds its own A_p0 (:190). */
int dkg_finalise_parties(dkg_ctx *ctx, size_t n, size_t t, const uint8_t *qualified, const uint8_t *reconstruct,
                         const uint8_t *r2_error, const uint8_t *r4_error, const uint8_t *disclosed, const uint8_t *A0,
                         const uint8_t *s, uint8_t *mpk, int32_t *status, int32_t *recovery_index);

/* ---- batches of independent ceremonies (BASELINE config 5: e.g. 10,000 ceremonies of n = 64) ----
 * B ceremonies with the same (n, t) and commitment key, each played as dkg_ceremony_run plays one
 * (full_valid_run, committee.rs:1518-1656): rounds 1-5 for every party of every ceremony.
 * Ceremony c's dealers are rows c*n .. c*n + n-1 of every [B*n]-row array; every output equals
 * what B separate single-ceremony calls return (the work of all B shares each kernel launch). */
typedef struct {
  /* host outputs; any pointer may be NULL */
  uint8_t *mpk;                 /* [B][32] MasterPublicKey per ceremony (committee.rs:726-805), as in
                                   dkg_ceremony_out; all zero for a ceremony with phase4_error */
  int32_t *n_qualified;         /* [B] */
  uint8_t *phase4_error;        /* [B] qualified minus reconstructable <= t (committee.rs:673-677) */
  uint8_t *qualified;           /* [B][n] */
  uint8_t *r2_error;            /* [B][n] receiver saw more than t complaints */
  uint8_t *r4_error;            /* [B][n] receiver saw fewer than t+1 honest dealers in round 4 */
  int32_t *complaints2;         /* [B][n] complaints raised by each receiver in round 2 */
  uint8_t *reconstruct;         /* [B][n] */
  uint8_t *final_share;         /* [B][n][32] */
  uint8_t *public_share;        /* [B][n][32] */
  uint8_t *dec2, *dec4;         /* [B][n dealer][n receiver] decision matrices (dec4 with SKIPPED) */
  /* device times, milliseconds (HIP events): round 1, the fused round-2/4 checks, round 3,
   * finalise (mpk incl. the round-4 combine), total */
  double ms_round1, ms_checks, ms_round3, ms_finalise, ms_total;
} dkg_batch_out;

/* Honest batch from device-resident coefficients d_a, d_b [B*n][t+1][32] (canonical scalars). */
int dkg_ceremony_batch_device(dkg_ctx *ctx, size_t B, size_t n, size_t t, const void *d_a, const void *d_b,
                              dkg_batch_out *out);
/* Receiver side of a batch from host broadcast values that may have been tampered with:
 * E, A [B*n][t+1][32]; s, s_prime [B*n][n][32] (row c*n + i = dealer i of ceremony c). */
int dkg_ceremony_batch_verify(dkg_ctx *ctx, size_t B, size_t n, size_t t, const uint8_t *E, const uint8_t *A,
                              const uint8_t *s, const uint8_t *s_prime, dkg_batch_out *out);

/* ---- full (encrypted-share) mode: the round-1 shares travel hybrid-encrypted
 * (committee.rs:164-172) under the members' communication keys and each receiver decrypts its own
 * (committee.rs:282-286).  Hybrid scheme (elgamal.rs:134-193): e1 = g*r, K = pk*r,
 * e2 = m XOR ChaCha20(key = Blake2b-512(K)[0..32], nonce = [32..44]); decryption K = sk*e1;
 * decrypted scalars are from_bits (groups.rs:29-36), reduced mod l on the device.
 * Ciphertext arrays are [D dealer][n recipient][2][32] with [..][0] = the randomness s' and
 * [..][1] = the share s (the reference encrypts the randomness first, committee.rs:171-172). ---- */
/* Seeded MemberCommunicationKey for n members (procedure_keys.rs:72-82):
 * sk_j = wide(ChaCha20Rng(BLAKE2b-256("dkg-amd/v1/member" || master || u32le ceremony || u32le j))),
 * pk_j = g*sk_j; returned SORTED by public-key bytes (committee.rs:134-135, procedure_keys.rs:26-40):
 * the party of index q+1 owns sk[q].  sk, pk [n][32]. */
int dkg_member_keys(dkg_ctx *ctx, const uint8_t master[32], uint32_t ceremony, size_t n, uint8_t *sk, uint8_t *pk);
/* Encryption randomness of dealers [d0, d0+D) for n recipients, continuing each dealer's seeded
 * stream after its 2(t+1) coefficient draws: r [D][n][2][32] (host), and the device variant for B
 * ceremonies (rows as dkg_dealer_coeffs_device). */
int dkg_enc_randomness(const uint8_t master[32], uint32_t ceremony, size_t d0, size_t D, size_t n, size_t t,
                       uint8_t *r);
int dkg_enc_randomness_device(dkg_ctx *ctx, const uint8_t master[32], uint32_t ceremony0, size_t B, size_t d0,
                              size_t D, size_t n, size_t t, void *d_r);
/* Hybrid-encrypt the share rows of D dealers (s, s_prime [D][n][32]) to the n recipients' keys
 * pk [n][32] with randomness r [D][n][2][32]: e1, ct [D][n][2][32].  DKG_E_DECODE if a key does
 * not decode. */
int dkg_encrypt_shares(dkg_ctx *ctx, size_t D, size_t n, const uint8_t *pk, const uint8_t *s, const uint8_t *s_prime,
                       const uint8_t *r, uint8_t *e1, uint8_t *ct);
/* Receivers' decryption with their secret keys sk [n][32]: s, s_prime [D][n][32];
 * ok [D][n][2] (may be NULL) = e1 decoded (a ciphertext that does not decode is missing data). */
int dkg_decrypt_shares(dkg_ctx *ctx, size_t D, size_t n, const uint8_t *sk, const uint8_t *e1, const uint8_t *ct,
                       uint8_t *s, uint8_t *s_prime, uint8_t *ok);
/* Whole ceremony in full mode from device coefficients d_a, d_b [n][t+1][32] and encryption
 * randomness d_r [n][n][2][32]; sk, pk = dkg_member_keys output (host).  With chunk streams
 * (dkg_ctx_set_streams > 1) the share evaluation, encryption and decryption run on a low-priority
 * stream beside the checks' difference tables (the checks wait for the decrypted shares), and the
 * members' key combs are kept on the ctx until the keys change; ms_round1 then times the
 * commitments and ms_round2 the rest up to the round-2/4 decisions.  With one stream: encryption in
 * ms_round1, decryption in ms_round2. */
int dkg_ceremony_run_full_device(dkg_ctx *ctx, size_t n, size_t t, const void *d_a, const void *d_b, const void *d_r,
                                 const uint8_t *sk, const uint8_t *pk, dkg_ceremony_out *out);
/* Receiver side of a full-mode ceremony from (possibly tampered) broadcast values: E, A
 * [n][t+1][32], e1, ct [n][n][2][32], the members' sorted secret keys sk [n][32].  A dealer with a
 * ciphertext that does not decode is missing data (DKG_MISSING in round 2).  out->s / s_prime
 * receive the decrypted shares. */
int dkg_ceremony_verify_full(dkg_ctx *ctx, size_t n, size_t t, const uint8_t *E, const uint8_t *A, const uint8_t *e1,
                             const uint8_t *ct, const uint8_t *sk, dkg_ceremony_out *out);

/* ---- full mode for batches of independent ceremonies ----
 * B ceremonies of n parties, each with its OWN member keys, run as dkg_ceremony_run_full_device /
 * dkg_ceremony_verify_full run one.  Row c*n + i of every [B*n]-row array is dealer i of ceremony c
 * (as in dkg_ceremony_batch_device); key arrays sk, pk are [B][n][32], recipient q of ceremony c
 * owning sk[c][q] / pk[c][q]; ciphertext arrays are [B*n dealer rows][n recipients][2][32] with
 * [..][0] = the randomness s' and [..][1] = the share s.  Every output equals what B separate
 * single-ceremony calls return.  Per-kernel device times of the last call, summed over its chunks:
 * dkg_ctx_phase_ms "bfull.enc_decode", "bfull.enc_tab" (the keys' radix-16 combs), "bfull.enc_e1"
 * (g*r), "bfull.enc_mul" (K = pk*r), "bfull.enc_encode", "bfull.enc_sym", "bfull.dec_decode",
 * "bfull.dec_mul" (K = sk*e1), "bfull.dec_encode", "bfull.dec_sym"; -1 for a phase the call did not
 * run. */
/* dkg_member_keys for ceremonies ceremony0 .. ceremony0 + B-1 (one fixed-base launch for all B*n
 * keys): ceremony c's rows equal dkg_member_keys(master, ceremony0 + c, n), sorted by public-key
 * bytes within the ceremony. */
int dkg_member_keys_batch(dkg_ctx *ctx, const uint8_t master[32], uint32_t ceremony0, size_t B, size_t n, uint8_t *sk,
                          uint8_t *pk);
/* dkg_encrypt_shares per ceremony: s, s_prime [B*n][n][32], r [B*n][n][2][32] (canonical scalars)
 * -> e1, ct [B*n][n][2][32]; recipient q of ceremony c is encrypted to pk[c][q] (only public keys
 * enter).  DKG_E_DECODE if a key does not decode. */
int dkg_encrypt_shares_batch(dkg_ctx *ctx, size_t B, size_t n, const uint8_t *pk, const uint8_t *s,
                             const uint8_t *s_prime, const uint8_t *r, uint8_t *e1, uint8_t *ct);
/* dkg_decrypt_shares per ceremony with sk [B][n][32]: s, s_prime [B*n][n][32]; ok [B*n][n][2] (may be
 * NULL) = e1 decoded. */
int dkg_decrypt_shares_batch(dkg_ctx *ctx, size_t B, size_t n, const uint8_t *sk, const uint8_t *e1, const uint8_t *ct,
                             uint8_t *s, uint8_t *s_prime, uint8_t *ok);
/* Honest full-mode batch from device coefficients d_a, d_b [B*n][t+1][32] and encryption randomness
 * d_r [B*n][n][2][32] (the layout dkg_enc_randomness_device(.., B, 0, n, n, t, ..) writes); sk, pk =
 * dkg_member_keys_batch output (host).  Share evaluation, encryption, the receivers' decryption, then
 * rounds 2-5 on the decrypted shares.  The hybrid stage runs on the context's stream: the encryption
 * is timed in ms_round1, the decryption in ms_checks. */
int dkg_ceremony_batch_full_device(dkg_ctx *ctx, size_t B, size_t n, size_t t, const void *d_a, const void *d_b,
                                   const void *d_r, const uint8_t *sk, const uint8_t *pk, dkg_batch_out *out);
/* Receiver side of a full-mode batch from (possibly tampered) host broadcast values: E, A
 * [B*n][t+1][32], e1, ct [B*n][n][2][32], sk [B][n][32].  A dealer with a ciphertext whose e1 does not
 * decode is missing data: DKG_MISSING for every receiver of its ceremony in round 2.  s_out,
 * s_prime_out ([B*n][n][32], may be NULL) receive the decrypted shares. */
int dkg_ceremony_batch_verify_full(dkg_ctx *ctx, size_t B, size_t n, size_t t, const uint8_t *E, const uint8_t *A,
                                   const uint8_t *e1, const uint8_t *ct, const uint8_t *sk, dkg_batch_out *out,
                                   uint8_t *s_out, uint8_t *s_prime_out);
/* The hybrid stage of the batch calls above runs in chunks of `ceremonies` ceremonies, so that its
 * scratch does not grow with B: per ceremony 2n^2 items x 352 B (the extended-form R and K, K's
 * encoding) and n keys x (160 B decoded + 80 KiB radix-16 comb) -- 8.1 MB at n = 64 -- plus the
 * decryption's odd-multiple table (40 KB per wave of a launch, at most 1.3 GB).  0 (default):
 * automatic, the largest count whose per-ceremony scratch fits 2 GiB (263 ceremonies at n = 64) and
 * whose decryption is one launch under the table's cap of 32,768 waves (256 at n = 64), at least 1.
 * Outputs do not depend on it. */
int dkg_ctx_set_batch_full_chunk(dkg_ctx *ctx, size_t ceremonies);

/* ---- complaint proofs: dl_equality/zkp.rs, broadcast.rs ----
 * enc [B][128] = one dealer->accuser ciphertext pair: e1_rand || ct_rand || e1_share || ct_share.
 * proof [192] = ProofOfMisbehaviour (broadcast.rs:181-186): share_key || randomness_key || c1 || r1
 * || c2 || r2, the two CorrectHybridDecrKeyZkp = DLEQ(g, e1, pk, K) proofs (challenge, response).
 * Verdicts (int32): 0 Ok (a valid complaint), 1 InvalidProofOfMisbehaviour, 2 FalseClaimedInequality,
 * 3 FalseClaimedEquality, -1 an input point does not decode. */
/* ProofOfMisbehaviour::generate (broadcast.rs:189-226) for B complaints by accusers with secret keys
 * sk [B][32]; nonces w [B][2][32]: w[0] for the share's proof (drawn first), w[1] the randomness's. */
int dkg_misbehaviour_prove(dkg_ctx *ctx, size_t B, const uint8_t *sk, const uint8_t *enc, const uint8_t *w,
                           uint8_t *proofs);
/* MisbehavingPartiesRound1::verify (broadcast.rs:50-99), including ProofOfMisbehaviour::verify
 * (:228-283) with its swapped-role check h*share + g*randomness (:271-274), reproduced as is:
 * accuser[b] = 1-based index, pk [B][32] the accuser's communication key, E [B][t+1][32] the
 * accused dealer's committed coefficients.  Requires dkg_env_init (h). */
int dkg_complaint1_verify(dkg_ctx *ctx, size_t B, size_t t, const uint32_t *accuser, const uint8_t *pk,
                          const uint8_t *enc, const uint8_t *E, const uint8_t *proofs, int32_t *result);
/* MisbehavingPartiesRound3::verify (broadcast.rs:105-135): the disclosed decrypted share and
 * randomness [B][32] must pass against E (else FalseClaimedEquality) and fail against A (else
 * FalseClaimedInequality). */
int dkg_complaint3_verify(dkg_ctx *ctx, size_t B, size_t t, const uint32_t *accuser, const uint8_t *share,
                          const uint8_t *randomness, const uint8_t *E, const uint8_t *A, int32_t *result);

/* ---- round-2 complaints as device batches (complaints.hip) and the qualified set they prove ----
 * In the reference a dealer leaves the qualified set only through a complaint that VERIFIES:
 * Phases<Phase2>::compute_qualified_set (committee.rs:370-398) runs MisbehavingPartiesRound1::verify
 * (broadcast.rs:50-99) on every broadcast complaint and clears the accused only on Ok. */
#define DKG_COMPLAINT_IGNORED 4 /* the accused published no phase-1 broadcast: skipped (committee.rs:377-380) */
/* ProofOfMisbehaviour::generate (broadcast.rs:189-226) for C complaints on the device.  Layouts as
 * dkg_misbehaviour_prove: sk [C][32] accuser keys, enc [C][128], w [C][2][32], proofs [C][192].
 * Byte-identical to it. */
int dkg_complaints_prove(dkg_ctx *ctx, size_t C, const uint8_t *sk, const uint8_t *enc, const uint8_t *w,
                         uint8_t *proofs);
/* Phases<Phase2>::compute_qualified_set (committee.rs:370-398) over C broadcast complaints of ONE
 * ceremony.  accuser[c], accused[c]: 1-based, DKG_E_ARG outside 1..n.  pk [n][32] sorted member keys.
 * E [n][t+1][32] phase-1 commitments.  fetched1 [n] (NULL = all present).
 * enc [C][128] = the ciphertext pair the ACCUSED broadcast to the accuser (not what the complaint
 * carries, broadcast.rs:57).  proofs [C][192].
 * verdict [C]: the codes of dkg_complaint1_verify (0 Ok, 1, 2, -1 a point does not decode), plus
 * DKG_COMPLAINT_IGNORED when the accused published no phase-1 broadcast (:377-380).
 * qualified [n] (may be NULL): 1 unless fetched1[i] == 0, E row i does not decode, or some complaint
 * against i has verdict 0.  Requires dkg_env_init (h). */
int dkg_complaints_verify(dkg_ctx *ctx, size_t n, size_t t, size_t C, const uint32_t *accuser,
                          const uint32_t *accused, const uint8_t *pk, const uint8_t *E, const uint8_t *fetched1,
                          const uint8_t *enc, const uint8_t *proofs, int32_t *verdict, uint8_t *qualified);
/* How dkg_complaints_verify evaluates P_i(j) = sum_k j^k E_i[k] (broadcast.rs:75-86): 0 automatic (per
 * accused dealer by its number of complaints, between 1 and 2), 1 always per-pair Horner in the exponent,
 * 2 always the difference tables of the accused rows, 4 always one wave per (row, index) item
 * (k_pair_eval: the shape of dkg_pair_eval_shape under dkg_ctx_set_receiver_chunk; a chunk that function
 * rejects makes the complaint call return DKG_E_ARG).  dkg_complaints3_verify, the proven ceremony
 * drivers and the sharded calls' fallback follow it too; the batch complaint stage does not.  3 is not a
 * mode (it is dkg_ctx_last_complaint_eval's code for "the calling pass") and stays DKG_E_ARG, as does
 * anything above 4.  Outputs do not depend on the mode. */
int dkg_ctx_set_complaint_eval(dkg_ctx *ctx, int mode);
/* dkg_ceremony_verify_full with the reference's rule for the qualified set (committee.rs:370-398):
 * decryption and the round-2/4 decisions run exactly as there (dec2, complaints2, r2_error keep their
 * meaning); then the C complaints (accuser, accused 1-based, proofs [C][192]; pk [n][32]) are verified
 * against this ceremony's own E, e1 and ct, and qualified[i] = row i is not MISSING and no complaint
 * against i has verdict 0.  SKIPPED in round 4, the round-3 sums, reconstruct, r4_error, phase4_error,
 * the public shares and mpk follow from that set.  verdict [C] as dkg_complaints_verify.
 * dissent [n] (may be NULL): dissent[j] = number of dealers i that receiver j rejected
 * (dec2[i][j] == DKG_REJECT) without a verdict-0 complaint by j against i among the C: such a party
 * has cleared i locally (committee.rs:311) while everyone else keeps it.  The outputs are the view
 * of the parties that are neither accuser nor accused. */
int dkg_ceremony_verify_full_complaints(dkg_ctx *ctx, size_t n, size_t t, const uint8_t *E, const uint8_t *A,
                                        const uint8_t *e1, const uint8_t *ct, const uint8_t *sk, const uint8_t *pk,
                                        size_t C, const uint32_t *accuser, const uint32_t *accused,
                                        const uint8_t *proofs, dkg_ceremony_out *out, int32_t *verdict,
                                        int32_t *dissent);

/* ---- round-4 complaints as a device batch (complaints.hip) and the reconstructable set they prove ----
 * In the reference a dealer enters reconstructable_set only in Phases<Phase4>::proceed
 * (committee.rs:625-688), through a broadcast MisbehavingPartiesRound3 complaint (broadcast.rs:104-144)
 * that VERIFIES, or whose accused published no phase-3 broadcast (:643).  Complaints against
 * disqualified dealers are ignored (:639), complaints that fail verify() too (:654-658). */
#define DKG_COMPLAINT_NO_PHASE3 5 /* the accused published no usable phase-3 broadcast: the complaint holds
                                     without verification (committee.rs:643) */
/* Phases<Phase4>::proceed's loop (committee.rs:636-670) over C broadcast complaints of ONE ceremony.
 * accuser[c], accused[c]: 1-based, DKG_E_ARG outside 1..n.  share, randomness [C][32]: the accuser's
 * decrypted pair as the complaint discloses it, read as dkg_complaint3_verify reads it (reduced mod
 * l).  E, A [n][t+1][32] the phase-1 / phase-3 commitments.  qualified [n] (NULL = all 1): the
 * round-2 qualified set.  fetched3 [n] (NULL = all 1): 0 = no phase-3 broadcast.
 * verdict [C], in this order of precedence:
 *   DKG_COMPLAINT_IGNORED (4)   qualified[accused] == 0 (:639);
 *   DKG_COMPLAINT_NO_PHASE3 (5) fetched3[accused] == 0, or the accused's A row does not decode (it
 *                               could not be deserialized: no broadcast) -- valid unverified (:643);
 *   -1                          the accused's E row does not decode;
 *   3 FalseClaimedEquality      g share + h randomness != sum_k j^k E_i[k] (broadcast.rs:129-130);
 *   2 FalseClaimedInequality    g share == sum_k j^k A_i[k] (:131-132);
 *   0                           a valid complaint.
 * 0, 2, 3 and -1 are dkg_complaint3_verify's codes.  reconstruct [n] (may be NULL): 1 when some
 * complaint against i has verdict 0 or 5 (:664-669); all zero for C == 0.  The evaluations follow
 * dkg_ctx_set_complaint_eval; outputs do not depend on it.  Requires dkg_env_init (h). */
int dkg_complaints3_verify(dkg_ctx *ctx, size_t n, size_t t, size_t C, const uint32_t *accuser,
                           const uint32_t *accused, const uint8_t *share, const uint8_t *randomness,
                           const uint8_t *E, const uint8_t *A, const uint8_t *qualified, const uint8_t *fetched3,
                           int32_t *verdict, uint8_t *reconstruct);
/* dkg_ceremony_verify_fetched with the reference's rule for the reconstructable set: round 2 keeps
 * the rejection rule (plaintext shares carry no ciphertexts to prove a round-1 complaint against),
 * the receivers' round-4 checks run as there (dec4, r4_error, the SKIPPED rows keep their meaning,
 * committee.rs:515-569), but reconstruct[i] = qualified[i] and some of the C4 broadcast complaints
 * (accuser4, accused4 1-based; share4, randomness4 [C4][32]) against i has verdict 0 or 5.
 * phase4_error, the disclosing parties, the recovered secrets and mpk follow from that set.
 * verdict4 [C4] as dkg_complaints3_verify with the ceremony's own qualified set.
 * finalise_status, recovery_index (may be NULL): the common outcome of the finalising parties in the
 * DKG_FIN_* codes -- OK; PHASE4_ERROR (phase4_error == 1); INSUFFICIENT with the first
 * reconstructed dealer (0-based) when fewer than t final parties disclose (:779-781); and
 * DKG_FIN_PANIC with recovery_index = i and mpk ALL ZERO when a qualified dealer i has no usable
 * phase-3 broadcast (fetched3[i] == 0 or an undecodable A row), is not in reconstruct, and so was
 * complained about by nobody: indexed_committed_shares[i] was never stored (:527-530) and every
 * party's finalise hits the expect at :791-795.  Dealers are visited in index order and the first
 * failure wins (:745-797).  The rejection-rule drivers cannot reach the PANIC state: there every
 * receiver's own rejection of such a dealer reconstructs it. */
int dkg_ceremony_verify_fetched_proven(dkg_ctx *ctx, size_t n, size_t t, const uint8_t *E, const uint8_t *A,
                                       const uint8_t *s, const uint8_t *s_prime, const uint8_t *fetched1,
                                       const uint8_t *fetched3, size_t C4, const uint32_t *accuser4,
                                       const uint32_t *accused4, const uint8_t *share4, const uint8_t *randomness4,
                                       dkg_ceremony_out *out, int32_t *verdict4, int32_t *finalise_status,
                                       int32_t *recovery_index);
/* dkg_ceremony_verify_full_complaints (qualified set by the proven round-1 complaints,
 * committee.rs:370-398) whose reconstructable set follows the proven round-4 complaints as in
 * dkg_ceremony_verify_fetched_proven (:625-688).  fetched3 [n] may be NULL (all present); the other
 * added arguments as there. */
int dkg_ceremony_verify_full_proven(dkg_ctx *ctx, size_t n, size_t t, const uint8_t *E, const uint8_t *A,
                                    const uint8_t *e1, const uint8_t *ct, const uint8_t *sk, const uint8_t *pk,
                                    size_t C, const uint32_t *accuser, const uint32_t *accused,
                                    const uint8_t *proofs, const uint8_t *fetched3, size_t C4,
                                    const uint32_t *accuser4, const uint32_t *accused4, const uint8_t *share4,
                                    const uint8_t *randomness4, dkg_ceremony_out *out, int32_t *verdict,
                                    int32_t *dissent, int32_t *verdict4, int32_t *finalise_status,
                                    int32_t *recovery_index);

/* ---- batches of ceremonies that decide by the proven complaints ----
 * dkg_ceremony_batch_verify / _verify_full keep the rejection rule in both rounds; these two calls
 * decide every ceremony of the batch as the single-ceremony *_proven calls decide one.  Complaints are
 * flat arrays over the whole batch: complaint c belongs to ceremony[c] (0-based, < B), accuser[c] and
 * accused[c] are 1-based within 1..n of that ceremony.  Any order: ceremonies interleaved, duplicates
 * allowed; verdicts are written in input order.  Every output for ceremony c -- each dkg_batch_out
 * field, verdict, verdict4, dissent[c], finalise_status[c], recovery_index[c] -- equals what the
 * matching single-ceremony call returns on ceremony c's slices and its own complaints in their
 * relative order: DKG_COMPLAINT_IGNORED against dealers round 2 disqualified, DKG_COMPLAINT_NO_PHASE3,
 * DKG_FIN_PANIC with that ceremony's mpk zeroed, DKG_FIN_INSUFFICIENT with the first reconstructed
 * dealer.  The proven rule holds for every ceremony of the call, also one without a complaint: there
 * nobody is disqualified except rows with missing data, and nobody is reconstructed.
 * B == 0 returns DKG_OK; C == 0 (C4 == 0) allows null complaint arrays; ceremony[c] >= B, an index
 * outside 1..n or a null required pointer returns DKG_E_ARG.  Requires dkg_env_init (h).
 * The complaints are verified on the device before the rounds, with no host synchronisation up to the
 * batch's one round trip: only the distinct accused rows are decoded a second time, the ciphertext
 * pairs are read from the batch's own e1 / ct, and P_i(j) is always one Horner walk per complaint --
 * dkg_ctx_set_complaint_eval does not apply.  Outputs do not depend on dkg_ctx_set_batch_full_chunk.
 * dkg_ctx_phase_ms "bproven.c4" / "bproven.c2": the device time of the round-4 / round-2 complaint
 * stage of the last such call (-1 for a stage it did not run).
 * dkg_complaints_prove takes one secret key per complaint, so it serves the complaints of any number
 * of ceremonies in one call as it is: there is no batch variant of it. */
/* dkg_ceremony_verify_fetched_proven for every ceremony of a batch.  fetched1, fetched3 [B*n] may be
 * NULL (all present).  verdict4 [C4]; finalise_status, recovery_index [B] (may be NULL). */
int dkg_ceremony_batch_verify_proven(dkg_ctx *ctx, size_t B, size_t n, size_t t, const uint8_t *E, const uint8_t *A,
                                     const uint8_t *s, const uint8_t *s_prime, const uint8_t *fetched1,
                                     const uint8_t *fetched3, size_t C4, const uint32_t *ceremony4,
                                     const uint32_t *accuser4, const uint32_t *accused4, const uint8_t *share4,
                                     const uint8_t *randomness4, dkg_batch_out *out, int32_t *verdict4,
                                     int32_t *finalise_status, int32_t *recovery_index);
/* dkg_ceremony_verify_full_proven for every ceremony of a batch.  sk, pk [B][n][32]; proofs [C][192];
 * verdict [C]; dissent [B][n] (may be NULL); fetched3 [B*n] (may be NULL); s_out, s_prime_out as
 * dkg_ceremony_batch_verify_full. */
int dkg_ceremony_batch_verify_full_proven(dkg_ctx *ctx, size_t B, size_t n, size_t t, const uint8_t *E,
                                          const uint8_t *A, const uint8_t *e1, const uint8_t *ct, const uint8_t *sk,
                                          const uint8_t *pk, size_t C, const uint32_t *ceremony,
                                          const uint32_t *accuser, const uint32_t *accused, const uint8_t *proofs,
                                          const uint8_t *fetched3, size_t C4, const uint32_t *ceremony4,
                                          const uint32_t *accuser4, const uint32_t *accused4, const uint8_t *share4,
                                          const uint8_t *randomness4, dkg_batch_out *out, uint8_t *s_out,
                                          uint8_t *s_prime_out, int32_t *verdict, int32_t *dissent, int32_t *verdict4,
                                          int32_t *finalise_status, int32_t *recovery_index);

/* ---- dealer-sharded ceremonies that decide by the proven complaints ----
 * dkg_ceremony_shard_verify_device / _shard_verify_full_device keep the rejection rule; these two calls
 * decide a rank's dealers as the single-ceremony *_proven calls decide all of them.  Every fact that
 * decides a complaint against dealer i lives on the rank that owns i (its E and A rows, its e1 / ct items
 * and their decode mask, its round-2 qualification, its fetched3 bit; the accusers' keys are the pk [n]
 * every rank takes), so each rank verifies the complaints against its own dealers and no exchange
 * precedes round 3.
 * Complaints: the WHOLE broadcast lists of the ceremony, host arrays as the single-ceremony calls take
 * them (accuser, accused 1-based; every rank passes the same lists, as a broadcast channel delivers
 * them).  The rank owns complaint c iff d0 < accused[c] <= d1 and verifies its owned complaints in their
 * relative input order, duplicates allowed, against its own rows: the ciphertext pair of complaint
 * (i, j) is items ((i - d0 - 1) n + j - 1) 2 + {0, 1} of d_e1 / d_ct (i, j 1-based), the commitments rows
 * i - d0 - 1 of d_E / d_A.  verdict [C] / verdict4 [C4] (host, out): the owned complaints' verdicts, codes
 * and precedence exactly those of dkg_complaints_verify and dkg_complaints3_verify (DKG_COMPLAINT_IGNORED
 * for a round-2 complaint against a dealer with fetched1 == 0 and for a round-4 complaint against a
 * dealer round 2 disqualified; DKG_COMPLAINT_NO_PHASE3); every other complaint reads
 * DKG_COMPLAINT_NOT_OWNED, which is below every real code, so that the element-wise maximum over the
 * ranks' arrays is the ceremony's verdict list (exactly one rank owns each complaint).
 * C == 0 / C4 == 0 allow null complaint arrays and still apply the proven rule: nobody is disqualified
 * except MISSING rows, nobody is reconstructed.  An index outside 1..n, or a null required pointer with
 * C > 0, is DKG_E_ARG.  d1 == d0 (a rank without dealers: world_size > n / 2 leaves some) works.
 * fetched1, fetched3: host [d1 - d0] intake masks of the rank's rows (NULL = all present), as
 * dkg_ceremony_verify_fetched: fetched1[i] == 0 makes a MISSING row, fetched3[i] == 0 an accusation by
 * every receiver in round 4 and verdict DKG_COMPLAINT_NO_PHASE3.
 * Outputs as the rejection-rule calls, with the rank's qualified set taken from the rule:
 * qualified[i] = row i is not MISSING and (full variant) no complaint against i has verdict 0 (plaintext
 * variant: no REJECT either, as dkg_ceremony_verify_fetched_proven); d_partial sums the shares of those
 * dealers; d_dec2 / d_dec4 / d_A0 are the raw rows as before (the combine applies SKIPPED), and the
 * decrypted shares are remembered for dkg_ceremony_shard_recon_device(d_s = NULL).
 * d_flags: device [flag_rows] u32, flag_rows >= d1 - d0 (pass dkg_shard_rows(n, world_size), the padded
 * block height the ranks gather; the entry point does not know world_size); rows past the rank's dealer
 * count are zero.  bit 0: some verdict-0 round-2 complaint against the row (never set by the plaintext
 * variant); bit 1: some round-4 complaint against it holds (verdict 0 or 5); bit 2: the row has no
 * usable phase-3 broadcast (fetched3 == 0 or an undecodable A row).
 * d_dissent (full variant; device [n] i32, may be NULL): the rank's partial of dissent[j] -- its dealers
 * that receiver j rejected without a verdict-0 complaint by j against them.
 * The complaint stage runs on the device inside the call, after the rank's checks and before the call's
 * one synchronisation; the owned complaints' index arrays and payloads go up in one staging copy.
 * Where P_i(j) comes from (dkg_ctx_last_complaint_eval): with dkg_ctx_set_complaint_eval(0) and the
 * fused group-check pipeline (dkg_ctx_set_overlap on, dkg_ctx_set_verify_mode 0) the rank's pass has
 * evaluated P^E_i(j) and P^A_i(j) for every receiver of every one of its dealers, and the complaints
 * read those elements -- source 3, "the calling pass": no Horner walk, no second set of tables.  With
 * protocol-order rounds or interpolation the pass does not hold both rounds' evaluations and the call
 * falls back to dkg_complaints_verify's switch (per accused row: Horner or tables); modes 1 and 2 of
 * dkg_ctx_set_complaint_eval force that switch's sources here too, and mode 4 sends the fallback's items
 * to the wave evaluator.  Source 3 exists only inside these
 * two calls and cannot be forced: dkg_ctx_set_complaint_eval(3) stays DKG_E_ARG.  Outputs do not depend
 * on any of this. */
#define DKG_COMPLAINT_NOT_OWNED (-2) /* the complaint's accused is another rank's dealer */
int dkg_ceremony_shard_verify_proven_device(dkg_ctx *ctx, size_t n, size_t t, size_t d0, size_t d1, const void *d_E,
                                            const void *d_A, const void *d_s, const void *d_s_prime,
                                            const uint8_t *fetched1, const uint8_t *fetched3, size_t C4,
                                            const uint32_t *accuser4, const uint32_t *accused4, const uint8_t *share4,
                                            const uint8_t *randomness4, void *d_dec2, void *d_dec4, void *d_A0,
                                            void *d_partial, size_t flag_rows, void *d_flags, int32_t *verdict4,
                                            double *ms_total);
int dkg_ceremony_shard_verify_full_proven_device(dkg_ctx *ctx, size_t n, size_t t, size_t d0, size_t d1,
                                                 const void *d_E, const void *d_A, const void *d_e1, const void *d_ct,
                                                 const uint8_t *sk, const uint8_t *pk, const uint8_t *fetched1,
                                                 const uint8_t *fetched3, size_t C, const uint32_t *accuser,
                                                 const uint32_t *accused, const uint8_t *proofs, size_t C4,
                                                 const uint32_t *accuser4, const uint32_t *accused4,
                                                 const uint8_t *share4, const uint8_t *randomness4, void *d_dec2,
                                                 void *d_dec4, void *d_A0, void *d_partial, size_t flag_rows,
                                                 void *d_flags, void *d_dissent, int32_t *verdict, int32_t *verdict4,
                                                 double *ms_total);
/* The evaluation source of the last sharded proven call on this ctx: 3 the calling pass, 1 Horner, 2
 * tables, 12 both of the fallback switch within one call, 4 the wave evaluator (the fallback under
 * dkg_ctx_set_complaint_eval(4)); 0 before the first such call and after one on a rank without dealers. */
int dkg_ctx_last_complaint_eval(const dkg_ctx *ctx);
/* dkg_shard_combine_packed_device for the proven calls: d_flags_g device [ws][R] u32 the gathered flag
 * words (R = dkg_shard_rows), d_dissent_g device [ws][n] i32 the gathered dissent partials (NULL with
 * dissent == NULL).  full != 0: the qualified set = the row is not MISSING and flag bit 0 is clear
 * (round2_device's cmask path, the functions the single-GPU drivers use); full == 0: from the rows, as
 * dkg_shard_combine_packed_device.  reconstruct[i] = qualified[i] && bit 1.  complaints2, r2_error,
 * r4_error keep their meaning and come from the rows; d_dec4 carries the SKIPPED rows of that qualified
 * set.  dissent [n] (host, may be NULL): the sum of the partials.  finalise_status / recovery_index (may
 * be NULL): the finalising parties' common outcome in the DKG_FIN_* codes as
 * dkg_ceremony_verify_fetched_proven reports it, a dealer's usable phase-3 broadcast taken from bit 2 --
 * OK, PHASE4_ERROR, INSUFFICIENT with the first reconstructed dealer, PANIC with the first qualified
 * dealer without a phase-3 broadcast that nobody complained about.  A caller that sees PANIC or
 * PHASE4_ERROR passes phase4_error = 1 to dkg_shard_finalise_device (an all-zero mpk, as the
 * single-ceremony call returns); INSUFFICIENT is what dkg_ceremony_shard_recon_device reports as
 * recovery_error. */
int dkg_shard_combine_proven_device(dkg_ctx *ctx, size_t n, size_t t, size_t world_size, const void *d_pack2_g,
                                    const void *d_pack4_g, const void *d_flags_g, const void *d_dissent_g, int full,
                                    void *d_dec2, void *d_dec4, dkg_shard_outcome *out, int32_t *dissent,
                                    int32_t *finalise_status, int32_t *recovery_index);
/* dkg_ceremony_verify_fetched_proven / dkg_ceremony_verify_full_proven over the shards of a multi-device
 * context, argument lists as there: each shard calls its sharded proven entry point on its host thread
 * with the whole complaint lists, packs its rows, and the flag words and dissent partials join the
 * peer-copy gather; the verdicts are merged on the host (exactly one shard owns each complaint).  Every
 * output -- out (E, A, s, s_prime NULL, as the other dkg_multi calls), verdict, verdict4, dissent,
 * finalise_status, recovery_index -- equals the single-context call's. */
int dkg_multi_ceremony_verify_proven(dkg_multi *m, size_t n, size_t t, const uint8_t *E, const uint8_t *A,
                                     const uint8_t *s, const uint8_t *s_prime, const uint8_t *fetched1,
                                     const uint8_t *fetched3, size_t C4, const uint32_t *accuser4,
                                     const uint32_t *accused4, const uint8_t *share4, const uint8_t *randomness4,
                                     dkg_ceremony_out *out, int32_t *verdict4, int32_t *finalise_status,
                                     int32_t *recovery_index);
int dkg_multi_ceremony_verify_full_proven(dkg_multi *m, size_t n, size_t t, const uint8_t *E, const uint8_t *A,
                                          const uint8_t *e1, const uint8_t *ct, const uint8_t *sk, const uint8_t *pk,
                                          size_t C, const uint32_t *accuser, const uint32_t *accused,
                                          const uint8_t *proofs, const uint8_t *fetched3, size_t C4,
                                          const uint32_t *accuser4, const uint32_t *accused4, const uint8_t *share4,
                                          const uint8_t *randomness4, dkg_ceremony_out *out, int32_t *verdict,
                                          int32_t *dissent, int32_t *verdict4, int32_t *finalise_status,
                                          int32_t *recovery_index);

/* ---- synthetic inputs: the seeded RNG convention ----
 * dealer seed = BLAKE2b-256("dkg-amd/v1/dealer" || master[32] || u32le ceremony || u32le dealer);
 * coefficients = ChaCha20Rng(seed): hiding b_0..b_t first, then sharing a_0..a_t (committee.rs:143-146),
 * each 64 bytes wide-reduced mod l (Scalar::random).  Host computation; a, b [D][t+1][32] for
 * dealers [d0, d0+D). */
int dkg_dealer_coeffs(const uint8_t master[32], uint32_t ceremony, size_t d0, size_t D, size_t t, uint8_t *a,
                      uint8_t *b);
/* The same convention on the GPU, for B ceremonies at once: row r in [0, B*D)
 * holds dealer d0 + r % D of ceremony ceremony0 + r / D; d_a, d_b are device buffers
 * [B*D][t+1][32].  Bit-identical to dkg_dealer_coeffs; keeps n = 4096 or 10,000-ceremony inputs
 * off the PCIe bus. */
int dkg_dealer_coeffs_device(dkg_ctx *ctx, const uint8_t master[32], uint32_t ceremony0, size_t B, size_t d0,
                             size_t D, size_t t, void *d_a, void *d_b);

#ifdef __cplusplus
}
#endif
#endif
