/*
 * flamingo_hip.h -- C ABI of libflamingo_hip.so, the MI355X (gfx950) engine
 * behind Flamingo's per-round mask-and-aggregate path.
 *
 * The reference (eniac/flamingo, pure Python) has no FFI; these entry points
 * replace the bodies of the reference's hot loops under an unchanged agent
 * surface.  Each function cites the reference code it stands in for
 * (paths relative to the reference root).
 *
 * Arithmetic: uint32 mod 2^32 everywhere (util/param.py:9 vector_type).
 * PRG(seed)[l] = LE32(ChaCha20_DJB(key=seed, nonce=0^8).keystream[4l:4l+4])
 *                ^ 0x64636261 (b"abcd", util/param.py:12,32).
 *
 * Conventions
 *  - Return 0 on success, a negative FLM_E* code on failure; the message is
 *    available from flm_last_error(ctx) (or flm_last_error(NULL) when no
 *    context could be created).  The Python layer raises RuntimeError, as the
 *    reference does on its own guard failures (SA_ServiceAgent.py:349,502).
 *  - seeds are K x 32 bytes (the reference's 32-byte ChaCha20 keys:
 *    m_i.to_bytes(32,'big') at SA_ServiceAgent.py:526, SHA-256 digests at
 *    :583-585); signs are K int8 in {+1,-1} (recon_symbol, :375-378; self
 *    masks are always -1, :536).
 *  - Host-pointer functions are synchronous: they copy in, compute on the
 *    GPU and copy out; no host pointer is retained after return.
 *  - *_dev functions take device pointers and enqueue work on `stream`
 *    (a hipStream_t; NULL = the HIP null stream) and return without waiting
 *    for earlier work: the small tables they upload (seg/signs, work items)
 *    go through a pool of pinned staging slots, each reused only after the
 *    launch that read it has completed.  The per-seed device tables a call
 *    builds come from a ring (8 per context) with the same rule: a table is
 *    rebuilt on a stream only after every launch on other streams that reads
 *    it has completed (or, when all are in use, that stream waits for them on
 *    the device), so calls of one context may run on any mix of streams with
 *    any seeds, without ordering by the caller.
 *  - One context per host thread; a context binds one GPU (one process per
 *    GPU).  Create it lazily, after any fork (SA_ServiceAgent.py:562 forks a
 *    multiprocessing.Pool).
 *  - Every entry point leaves the calling thread's current HIP device as it
 *    found it: a call selects its context's device (or each rank's, for a
 *    group or store) only for its own duration.
 */
#ifndef FLAMINGO_HIP_H
#define FLAMINGO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FLM_OK 0
#define FLM_EINVAL (-1)   /* bad argument (length mismatch, sign not +-1, alignment) */
#define FLM_EHIP (-2)     /* HIP runtime error */
#define FLM_ENOMEM (-3)   /* device or pinned allocation failed */
#define FLM_ERANGE (-4)   /* slot range beyond 2^36 (block counter high word must be 0): a window of n slots from
                             slot0 needs slot0 <= 2^36 and n <= 2^36 - slot0 (no 64-bit sum that could wrap) */

typedef struct flm_ctx flm_ctx;

/* ------------------------------------------------------------ lifecycle */
int flm_device_count(void);
/* Bind a context to HIP device `device` and create its stream. */
int flm_init(flm_ctx **out, int device);
void flm_free(flm_ctx *ctx);
const char *flm_last_error(const flm_ctx *ctx);
/* The context's own non-blocking stream (a hipStream_t): the host-pointer calls and
 * the flm_group rounds run on it, so a caller can order its own streams against them. */
void *flm_ctx_stream(flm_ctx *ctx);
/* Library / kernel build identification string (static storage). */
const char *flm_version(void);

/* ---------------------------------------------------- host-memory path */

/* Server round: replaces SA_ServiceAgent.report_process's partial sum
 * (agent/flamingo/SA_ServiceAgent.py:346-350) and reconstruction_process's
 * self-mask and dropout-pair unmask + final combine (:529-540, :587-605):
 *   out[l] = sum_{i<N} rows[i][l] + sum_{k<K} signs[k] * PRG(seeds[k])[l]
 * rows: N host pointers to L uint32 each (the VECTOR bodies, :210). */
int flm_aggregate_unmask(flm_ctx *ctx, const uint32_t *const *rows, int N, const uint8_t *seeds,
                         const int8_t *signs, int K, size_t L, uint32_t *out);

/* Client masking, batched over N clients: replaces SA_ClientAgent.sendVectors's
 * mask expansion and composition (agent/flamingo/SA_ClientAgent.py:246-324):
 *   out[i][l] = x[i][l] + sum_{k in [seg[i], seg[i+1])} signs[k] * PRG(seeds[k])[l]
 * x: N x L row-major uint32, or NULL for the reference's all-ones input (:304).
 * out: N x L row-major. */
int flm_client_mask(flm_ctx *ctx, const uint32_t *x, int N, const int64_t *seg, const uint8_t *seeds,
                    const int8_t *signs, size_t L, uint32_t *out);

/* Standalone PRG expansion: out[k][l] = PRG(seeds[k])[slot0 + l], K x L
 * row-major (the idiom at SA_ClientAgent.py:248-250 / SA_ServiceAgent.py:533-535
 * for a whole batch).  slot0 must be a multiple of 16. */
int flm_prg_expand(flm_ctx *ctx, const uint8_t *seeds, int K, size_t L, uint64_t slot0, uint32_t *out);

/* acc[l] += sum_k signs[k] * PRG(seeds[k])[slot0 + l], in place on a host
 * vector (the mi_vec / cancel_vec loops, SA_ServiceAgent.py:530-536, 595-603,
 * on a slot window).  slot0 must be a multiple of 16. */
int flm_mask_accumulate(flm_ctx *ctx, const uint8_t *seeds, const int8_t *signs, int K, uint32_t *acc,
                        size_t L, uint64_t slot0);

/* ChaCha20(key, nonce).encrypt(in) from block `counter` on, byte-exact, any
 * length: the PRF/PRG calls of util/param.py:44-46 (choose_committee) and
 * :63-76 (findNeighbors), computed on the GPU. */
int flm_chacha20_xor(flm_ctx *ctx, const uint8_t key[32], const uint8_t nonce[8], uint64_t counter,
                     const uint8_t *in, uint8_t *out, size_t n);

/* -------------------------------------------------- device-resident path */

/* Device-resident server round over a slot window, for single- and multi-GPU use:
 *   out[l]  = sum_{i<N} rows[i*row_pitch + l]                  for l in [0, L)
 *           + sum_k signs[k] * PRG(seeds[k])[prg_slot0 + l]    for l in [mask_lo, mask_hi)
 * (mod 2^32).  With mask_lo=0, mask_hi=L, prg_slot0=0 this is the whole
 * round; on G GPUs each rank passes its own client rows and its own slot
 * shard [mask_lo, mask_hi) and the partial vectors are then reduce-scattered.
 * Requirements: row_pitch % 4 == 0 and row_pitch >= round_up(L, 4);
 * rows and out 16-byte aligned; mask_lo % 16 == 0; prg_slot0 % 16 == 0;
 * prg_slot0 + mask_hi <= 2^36.  d_seeds: K x 32 bytes, d_signs: K int8 (+-1).
 * Enqueued on `stream`; nothing is synchronised. */
int flm_aggregate_unmask_dev(flm_ctx *ctx, const uint32_t *d_rows, size_t row_pitch, int N,
                             const uint8_t *d_seeds, const int8_t *d_signs, int K, size_t L,
                             size_t mask_lo, size_t mask_hi, uint64_t prg_slot0, uint32_t *d_out,
                             void *stream);

/* The same round split in its two launches, so a caller can time the
 * dominant kernel alone: flm_seed_table_dev builds the context's per-seed
 * schedule (ChaCha key words, sign, counter-independent first-round words)
 * from device seeds/signs; flm_aggregate_dev then runs the row-sum + unmask
 * kernel against that table (K must match the table), on any stream: a read
 * on another stream than the table's build waits for the build on the device.
 * The table stays published until the context's next call that builds a seed
 * table (any *_dev round, expansion, client masking, pair units, or another
 * flm_seed_table_dev); flm_aggregate_dev then fails with FLM_EINVAL rather
 * than unmask against other seeds.  Same requirements as flm_aggregate_unmask_dev. */
int flm_seed_table_dev(flm_ctx *ctx, const uint8_t *d_seeds, const int8_t *d_signs, int K, void *stream);
int flm_aggregate_dev(flm_ctx *ctx, const uint32_t *d_rows, size_t row_pitch, int N, int K, size_t L,
                      size_t mask_lo, size_t mask_hi, uint64_t prg_slot0, uint32_t *d_out, void *stream);

/* Device-resident client masking (flm_client_mask on device buffers).  seg and
 * signs are host arrays (they size the launch); seeds, x and out are device
 * pointers; x may be NULL (all-ones input).  x and out rows use `pitch`. */
int flm_client_mask_dev(flm_ctx *ctx, const uint32_t *d_x, size_t pitch, int N, const int64_t *seg,
                        const uint8_t *d_seeds, const int8_t *signs, size_t L, uint32_t *d_out,
                        void *stream);

/* ------------------------------------------------------ fixed-point codec */

/* Float updates in, float mean out: the fixed-point codec around the ring sum, for the use the
 * reference names at agent/flamingo/SA_ClientAgent.py:300-304 ("For machine learning, replace it
 * with model weights").  Parameters: frac_bits f in 0..30; clip c, a finite float32 > 0.
 *   encode(x): NaN -> 0; xc = min(max(x, -c), c); t = xc * 2^f in float32 (exact);
 *     nearest (no dither seed): q = int32(rint(t)), ties to even;
 *     stochastic (a 32-byte dither seed per client): ti = trunc(t), fr = |t - ti|,
 *       thr = uint32(trunc(fr * 2^32)), r = PRG(dither_i)[l], q = int32(ti) + sgn(t) * [r < thr];
 *     the ring word is uint32(q), two's complement.  An element is *clipped* when it was NaN or |x| > c.
 *   decode(s, count) = float32(float64(int32(s)) / (float64(count) * 2^f)).
 * Headroom for n contributors: n * ceil(c * 2^f) <= 2^31 - 1, or the sum can wrap.
 *
 * flm_codec_check: FLM_EINVAL for f outside 0..30, a clip that is not finite and positive, or
 * n_clients < 1; FLM_ERANGE outside the headroom; needs no context and no device.  What a caller,
 * or the agents' server (SA_ServiceAgent.py:538-540, 605: its final sum), calls with the real n. */
int flm_codec_check(int frac_bits, float clip, int64_t n_clients);

/* Client masking of float input, the encoding fused in (SA_ClientAgent.py:300-324):
 *   out[i][l] = encode(x[i][l]) + sum_{k in [seg[i], seg[i+1])} signs[k] * PRG(seeds[k])[l]
 * x: N x L row-major float32 (required); dither: N x 32 bytes, or NULL for nearest-even;
 * clipped: N counts of clipped elements (written), or NULL.  The encoded word is never stored
 * unmasked.  flm_client_mask's rules for seg and signs; the codec's rules with n = 1. */
int flm_client_encode_mask(flm_ctx *ctx, const float *x, int N, const int64_t *seg, const uint8_t *seeds,
                           const int8_t *signs, size_t L, int frac_bits, float clip, const uint8_t *dither,
                           uint32_t *out, uint32_t *clipped);
/* The same on device buffers (SA_ClientAgent.py:300-324), enqueued on `stream` (NULL: the null
 * stream); nothing is synchronised.  seg and signs are host arrays; x rows are x_pitch floats
 * apart, out rows out_pitch words (each a multiple of 4 and >= round_up(L, 4)); x and out 16-byte
 * aligned.  Whatever the padding of an x row holds is not read as input.  d_clipped (N words or
 * NULL) is zeroed on the stream first. */
int flm_client_encode_mask_dev(flm_ctx *ctx, const float *d_x, size_t x_pitch, int N, const int64_t *seg,
                               const uint8_t *d_seeds, const int8_t *signs, size_t L, int frac_bits, float clip,
                               const uint8_t *d_dither, uint32_t *d_out, size_t out_pitch, uint32_t *d_clipped,
                               void *stream);
/* out[l] = decode(sum[l], count): the server's final sum (SA_ServiceAgent.py:538-540, 605) as the
 * mean of `count` contributors; count = 1 gives the sum.  FLM_EINVAL for count < 1 or f outside 0..30. */
int flm_decode_sum(flm_ctx *ctx, const uint32_t *sum, size_t L, int frac_bits, int64_t count, float *out);
/* The same on device buffers (SA_ServiceAgent.py:538-540, 605), 16-byte aligned; d_out may alias d_sum. */
int flm_decode_sum_dev(flm_ctx *ctx, const uint32_t *d_sum, size_t L, int frac_bits, int64_t count, float *d_out,
                       void *stream);

/* ------------------------------------------------ packed fixed-point codec */

/* Several parameters per ring word: pack P = 2 or 4 fields of W = 32 / P bits (pack = 1 is the calls
 * above; any other value is FLM_EINVAL).  A quantised update needs far fewer than 32 bits, and a round
 * over L parameters becomes the same round over Lw = ceil(L / P) words: rows, masks and wire bytes
 * fall by P.  With B = ceil(c * 2^f), the integer of the headroom rule above:
 *   field: u = q + B, q the codec's encode(x) (|q| <= B in both roundings), so u is in [0, 2B];
 *     stochastic rounding takes r = PRG(dither_i)[l], indexed by parameter l, not by word;
 *   word l' = sum_{j < P} u[P * l' + j] << (W * j): consecutive parameters, parameter P * l' in the low
 *     field; fields of parameters >= L hold 0, are not counted as clipped and are never read as input;
 *   masks are full 32-bit words indexed by word, PRG(seed)[l'], as before.
 *   decode(S, count): s_j = (S >> W * j) & (2^W - 1),
 *     out[P * l' + j] = float32(float64(s_j - count * B) / (float64(count) * 2^f)) for P * l' + j < L:
 *     bit for bit the unpacked decode of the unpacked sum whenever both codecs have headroom.
 * Headroom for n contributors: n * 2B <= 2^W - 1, in integers, so that no field of the sum carries into
 * its neighbour; outside it FLM_ERANGE.  At (f = 7, c = 1, P = 2) that is n <= 255, at (4, 1, 2)
 * n <= 2047; P = 4 serves small cohorts only: n <= 31 at (2, 1, 4), n <= 127 at (0, 1, 4).
 *
 * flm_codec_check_packed: flm_codec_check's refusals, FLM_EINVAL for pack not 2 or 4, FLM_ERANGE outside
 * the packed headroom; no context, no device.  The agents' server (SA_ServiceAgent.py:538-540, 605: its
 * final sum) calls it with the real n. */
int flm_codec_check_packed(int frac_bits, float clip, int pack, int64_t n_clients);

/* Client masking of float input into packed words (SA_ClientAgent.py:300-324):
 *   out[i][l'] = word l' of x[i] + sum_{k in [seg[i], seg[i+1])} signs[k] * PRG(seeds[k])[l']
 * x: N x L float32; out: N x ceil(L / pack) words; dither, clipped as flm_client_encode_mask's.  The
 * encoded word is never stored unmasked.  The packed headroom rule with n = 1. */
int flm_client_encode_pack_mask(flm_ctx *ctx, const float *x, int N, const int64_t *seg, const uint8_t *seeds,
                                const int8_t *signs, size_t L, int frac_bits, float clip, int pack,
                                const uint8_t *dither, uint32_t *out, uint32_t *clipped);
/* The same on device buffers (SA_ClientAgent.py:300-324), enqueued on `stream`; nothing is synchronised.
 * x rows are x_pitch floats apart (a multiple of 4, >= round_up(L, 4)), out rows out_pitch words (a
 * multiple of 4, >= round_up(ceil(L / pack), 4)); both 16-byte aligned.  The padding of an x row is not
 * read as input and the padding of an out row is not written. */
int flm_client_encode_pack_mask_dev(flm_ctx *ctx, const float *d_x, size_t x_pitch, int N, const int64_t *seg,
                                    const uint8_t *d_seeds, const int8_t *signs, size_t L, int frac_bits,
                                    float clip, int pack, const uint8_t *d_dither, uint32_t *d_out,
                                    size_t out_pitch, uint32_t *d_clipped, void *stream);
/* out[0..L) = decode(sum[0..ceil(L / pack)), count): the server's final sum (SA_ServiceAgent.py:538-540,
 * 605) as the mean of `count` contributors.  The packed headroom rule with n = count. */
int flm_decode_unpack(flm_ctx *ctx, const uint32_t *sum, size_t L, int frac_bits, float clip, int pack,
                      int64_t count, float *out);
/* The same on device buffers (SA_ServiceAgent.py:538-540, 605), 16-byte aligned; d_out is not d_sum (it
 * is `pack` times as long). */
int flm_decode_unpack_dev(flm_ctx *ctx, const uint32_t *d_sum, size_t L, int frac_bits, float clip, int pack,
                          int64_t count, float *d_out, void *stream);

/* ------------------------------------- distributed-DP noise in the codec */

/* Distributed differential privacy by the binomial mechanism (Agarwal et al., "cpSGD", NeurIPS 2018):
 * every client adds a small share of integer noise to its quantised update before masking, so only
 * the sum of the shares ever appears in what the server unmasks.  The reference's learning example
 * does the local half on the host (agent/examples/crypto/PPFL_ClientAgent.py:219-221, 274-285: Laplace
 * noise added to the weights before secure aggregation); here the share is drawn inside the
 * encode-mask kernel (SA_ClientAgent.py:300-324), so the noised word exists only in registers.
 *   noise_bits b: fair coin flips per parameter per client; 0 = off, else even, 2 <= b <= 1024.
 *     m = ceil(b / 32) draws, r = b mod 32.
 *   noise: one 32-byte seed per client, N x 32 bytes; secret and fresh per iteration, like the dither
 *     seed.  The stream is PRG(noise_i), the PRG of every mask and of the dither.
 *   draw d < m of parameter l: w(l, d) = PRG(noise_i)[16 * (m * (l / 16) + d) + l % 16]; if r != 0 the
 *     last draw (d = m - 1) is ANDed with 2^r - 1.  Block-interleaved: ChaCha block m * beta + d gives
 *     draw d of all 16 parameters of parameter block beta.  Indexed by parameter, not by ring word, in
 *     every pack mode, as the dither is.
 *   Z_i[l] = sum_d popcount(w(l, d)) - b / 2: in [-b / 2, b / 2], mean 0, variance b / 4.
 *   q' = q + Z, q the codec's encode in either rounding.  pack = 1: the ring word is uint32(q').
 *     pack = 2, 4: the field is u = q' + B_n, B_n = B + b / 2, B = ceil(c * 2^f), so u is in [0, 2 B_n].
 *     Parameters >= L get no noise: their fields hold 0, they are not counted as clipped and never
 *     stored.  The clipped count is that of the same call without noise.
 *   decode: pack = 1: flm_decode_sum as it is (the noise has zero mean); packed: the packed decode with
 *     B_n in B's place.
 * Headroom, worst case, in exact integers, FLM_ERANGE outside it: pack = 1: n * B_n <= 2^31 - 1; packed:
 * n * 2 * B_n <= 2^W - 1, W = 32 / pack.  (f = 4, c = 1, P = 2, b = 30): B_n = 31, n <= 1057; (2, 1, 4, 2):
 * B_n = 5, n <= 25; (7, 1, 2) with n = 255 has no room for any noise.  The bound is worst case, every coin
 * of every client on one side; a cohort it refuses decodes modulo the field instead ("decode modulo the field" below,
 * which bounds no wrap probability either).  Length: m * ceil(L / 16) <= 2^32,
 * because the noise stream's block counter has no high word; else FLM_ERANGE.
 * The decoded mean over |U| contributors carries noise of standard deviation
 * sqrt(|U| * b) / (2 * |U| * 2^f); a dropped client's share is simply absent.  Converting b to an
 * (epsilon, delta) is the caller's business.
 *
 * flm_codec_check_noise (SA_ClientAgent.py:300-324; PPFL_ClientAgent.py:219-221, 274-285): pack 1, 2 or
 * 4; FLM_EINVAL for any other pack and for noise_bits odd, negative or > 1024, and the refusals of
 * flm_codec_check (pack = 1) or flm_codec_check_packed; FLM_ERANGE outside the headroom, and, when
 * L_params > 0, outside the length rule.  No context, no device.  noise_bits = 0: those checks alone. */
int flm_codec_check_noise(int frac_bits, float clip, int pack, int noise_bits, int64_t n_clients, uint64_t L_params);

/* Client masking of float input with the client's noise share (SA_ClientAgent.py:300-324;
 * agent/examples/crypto/PPFL_ClientAgent.py:219-221, 274-285): flm_client_encode_pack_mask's arguments,
 * pack 1 (rows of L words, as flm_client_encode_mask), 2 or 4, and noise_bits with the N x 32 bytes of
 * `noise`.  noise_bits = 0 runs flm_client_encode_mask or flm_client_encode_pack_mask, `noise` is
 * ignored and the result is theirs bit for bit; noise_bits > 0 with `noise` NULL is FLM_EINVAL, refused
 * before anything is launched.  The rule above with n = 1 and L. */
int flm_client_encode_noise_mask(flm_ctx *ctx, const float *x, int N, const int64_t *seg, const uint8_t *seeds,
                                 const int8_t *signs, size_t L, int frac_bits, float clip, int pack,
                                 const uint8_t *dither, int noise_bits, const uint8_t *noise, uint32_t *out,
                                 uint32_t *clipped);
/* The same on device buffers (SA_ClientAgent.py:300-324; PPFL_ClientAgent.py:219-221, 274-285), enqueued
 * on `stream`; nothing is synchronised, seg and signs are staged through the slot pool.  Pitches and
 * alignment as flm_client_encode_pack_mask_dev's; d_noise: N x 32 bytes on the device. */
int flm_client_encode_noise_mask_dev(flm_ctx *ctx, const float *d_x, size_t x_pitch, int N, const int64_t *seg,
                                     const uint8_t *d_seeds, const int8_t *signs, size_t L, int frac_bits,
                                     float clip, int pack, const uint8_t *d_dither, int noise_bits,
                                     const uint8_t *d_noise, uint32_t *d_out, size_t out_pitch,
                                     uint32_t *d_clipped, void *stream);
/* flm_decode_unpack of noised packed rows (SA_ClientAgent.py:300-324 and PPFL_ClientAgent.py:219-221,
 * 274-285 made the input; SA_ServiceAgent.py:538-540, 605 the sum): pack 2 or 4, the bias count * B_n.
 * The headroom rule above with n = count. */
int flm_decode_unpack_noise(flm_ctx *ctx, const uint32_t *sum, size_t L, int frac_bits, float clip, int pack,
                            int noise_bits, int64_t count, float *out);
/* The same on device buffers (SA_ClientAgent.py:300-324; PPFL_ClientAgent.py:219-221, 274-285). */
int flm_decode_unpack_noise_dev(flm_ctx *ctx, const uint32_t *d_sum, size_t L, int frac_bits, float clip, int pack,
                                int noise_bits, int64_t count, float *d_out, void *stream);

/* ------------------------------ discrete Gaussian noise shares, sampled from a cumulative table */

/* The noise share of the distributed discrete Gaussian mechanism (Kairouz, Liu, Steinke, ICML 2021, Algorithm 1)
 * in the place of the binomial one above (SA_ClientAgent.py:300-324; PPFL_ClientAgent.py:219-221, 274-285): the
 * client's share Z is sampled inside the encode-mask kernel from a cumulative table the caller built.  A fixed
 * number of table probes per parameter: nothing loops on data, and the result is a function of the seed.  Normative:
 *   tail tau: an integer, 1 <= tau <= 512; Z lies in [-tau, tau].  tau = 0 is not "off": it is refused
 *     (FLM_EINVAL); the calls without noise exist.
 *   cdt[0 .. T - 1]: uint64, non-decreasing, T = 2 tau (at most 8 KiB).  cdt[j] stands for 2^64 P(Z <= j - tau):
 *     a draw below it gives a sample <= j - tau.  The sample is defined by the count alone (below); with it
 *     P(Z = -tau) = cdt[0] / 2^64, P(Z = tau) = 1 - cdt[T - 1] / 2^64, and cdt[0] = 0 means "-tau never occurs".
 *     For a discrete Gaussian of parameter sigma truncated to |Z| <= tau, cdt[j] = floor(2^64 sum_{k = -tau}^{j -
 *     tau} w(k) / sum_{k = -tau}^{tau} w(k)), w(k) = exp(-k^2 / (2 sigma^2)); tau = 1 with cdt = {2^63, 2^63} gives
 *     -1 and +1 with probability 1/2 each and never 0.  The library takes the table and does not build it
 *     (flamingo_amd/dgauss.py does).
 *   noise: one 32-byte seed per client, as above.  With beta = l / 16, the draw of parameter l is
 *     u(l) = PRG(noise_i)[16 * (2 beta) + l % 16] * 2^32 + PRG(noise_i)[16 * (2 beta + 1) + l % 16]: ChaCha
 *     block 2 beta holds the high words of parameter block beta, block 2 beta + 1 the low words (the binomial
 *     stream's layout at m = 2).  Indexed by parameter in every pack mode.
 *   z(l) = #{ j < T : cdt[j] <= u(l) } - tau, the compare a 64-bit unsigned one.
 *   q' = q + z, q the codec's encode in either rounding (what flm_round_select counts).  pack = 1: the ring word is
 *     uint32(q').  pack = 2, 4: the field is q + B + (z + tau), bias B_n = B + tau.  Parameters >= L get no noise:
 *     their fields hold 0 and they are never stored.  The clipped count is that of the call without noise.
 *   decode: rows of these calls decode as rows of flm_client_encode_noise_mask with noise_bits = 2 tau do:
 *     pack = 1 with flm_decode_sum[_dev], packed with flm_decode_unpack_noise[_dev] or
 *     flm_store_unmask_unpack_noise_f32 at noise_bits = 2 * tail.  There are no decode calls of its own.
 * Headroom, worst case, in exact integers, FLM_ERANGE outside it: the rule above with B_n = B + tau: pack = 1:
 * n * B_n <= 2^31 - 1; packed: n * 2 * B_n <= 2^W - 1.  Length: 2 * ceil(L / 16) <= 2^32, else FLM_ERANGE.
 * The host form refuses a table that decreases anywhere (FLM_EINVAL).  The device form cannot see its table:
 * whatever the table holds, every probe reads inside it and the count stays in [0, T], so no field leaves its
 * headroom.  Privacy accounting (sigma, the mass beyond tau, the sensitivity flm_round_bound gives) is the caller's.
 *
 * flm_codec_check_gauss: FLM_EINVAL for tail outside 1..512 and the refusals of flm_codec_check_noise's codec
 * (pack 1, 2 or 4); FLM_ERANGE outside the headroom and, when L_params > 0, the length rule.  No context. */
int flm_codec_check_gauss(int frac_bits, float clip, int pack, int tail, int64_t n_clients, uint64_t L_params);
/* FLM_EINVAL for cdt NULL, tail outside 1..512 or cdt[j] < cdt[j - 1] for some 0 < j < 2 tail
 * (PPFL_ClientAgent.py:219-221, 274-285: the noise a client adds).  No context, no device. */
int flm_dgauss_check_table(const uint64_t *cdt, int tail);
/* flm_client_encode_noise_mask with the table in the place of noise_bits (SA_ClientAgent.py:300-324;
 * PPFL_ClientAgent.py:219-221, 274-285): cdt 2 * tail entries, checked as flm_dgauss_check_table does; noise
 * N x 32 bytes; either NULL is FLM_EINVAL.  The rule above with n = 1 and L, refused before anything is launched. */
int flm_client_encode_gauss_mask(flm_ctx *ctx, const float *x, int N, const int64_t *seg, const uint8_t *seeds,
                                 const int8_t *signs, size_t L, int frac_bits, float clip, int pack,
                                 const uint8_t *dither, int tail, const uint64_t *cdt, const uint8_t *noise,
                                 uint32_t *out, uint32_t *clipped);
/* The same on device buffers (SA_ClientAgent.py:300-324; PPFL_ClientAgent.py:219-221, 274-285), as
 * flm_client_encode_noise_mask_dev; d_cdt: 2 * tail uint64 on the device, 8-byte aligned ("cdt must be 8-byte
 * aligned", FLM_EINVAL, otherwise), not looked at by the host. */
int flm_client_encode_gauss_mask_dev(flm_ctx *ctx, const float *d_x, size_t x_pitch, int N, const int64_t *seg,
                                     const uint8_t *d_seeds, const int8_t *signs, size_t L, int frac_bits,
                                     float clip, int pack, const uint8_t *d_dither, int tail, const uint64_t *d_cdt,
                                     const uint8_t *d_noise, uint32_t *d_out, size_t out_pitch,
                                     uint32_t *d_clipped, void *stream);

/* ------------------------------ decode modulo the field: centred, carry-aware unpacking of packed sums */

/* The server's half of the distributed discrete Gaussian mechanism (Kairouz, Liu, Steinke, ICML 2021, Algorithm 1): the
 * sum is taken modulo m and mapped back to [-m/2, m/2).  Here m = M = 2^W per packed field: a field of the summed word
 * is a residue mod M, and a field that outgrew its W bits has carried into the one above it, which the decode follows
 * (SA_ServiceAgent.py:538-540, 605: the final sum).  The encode calls, the wire format and the ring sum are untouched:
 * every client still encodes under the rule with n = 1.  Normative:
 *   pack P in {2, 4}, W = 32 / P, M = 2^W, H = 2^(W - 1).
 *   B_n = ceil(c * 2^f) + noise_bits / 2, as above (the table mode passes noise_bits = 2 * tail).
 *   count = n >= 1; cb = (n * B_n) mod 2^32.
 *   For a summed word S the true field sums are T_j = Q_j + n * B_n, Q_j the signed sum of the clients' q' at
 *     parameter P * l' + j, and S = sum_j T_j << (W * j) mod 2^32: carries between fields are allowed.
 *   The decode works upward through the fields, field 0 first:
 *     r_0 = S
 *     for j = 0 .. P - 1:
 *       d_j  = (r_j - cb) mod 2^32
 *       v_j  = d_j mod M
 *       Qh_j = v_j - M * [v_j >= H]                      in [-H, H - 1]
 *       r_{j+1} = ((d_j - Qh_j) mod 2^32) >> W           logical shift; the low W bits of the difference are 0
 *       out[P * l' + j] = float32(float64(Qh_j) / (float64(n) * 2^f))    for P * l' + j < L
 *     the division and the single rounding are flm_decode_unpack's.
 * Properties:
 *   1. If every Q_j of the word lies in [-H, H - 1], then Qh_j = Q_j, whatever n * B_n is: also when T_j >= M, and when
 *      n * B_n >= 2^32.
 *   2. Whenever the worst-case rule n * 2 * B_n <= M - 1 holds, the output is flm_decode_unpack_noise's, bit for bit.
 *   3. Wrapping is defined, not undefined: with k_{-1} = 0, Qh_j = centred((Q_j + k_{j-1}) mod M) and
 *      k_j = (Q_j + k_{j-1} - Qh_j) / M.  A wrapped field is off by a multiple of M and hands k (a few units of
 *      2^-f / n in the mean) to the field above it.  The sum cannot reveal a wrap: a wrapped Q_j and the in-range value
 *      it is congruent to give the same word.  The library bounds nothing about the probability of a wrap; it reports
 *      how close the decoded fields came (below), and the caller chooses the parameters.
 * Near-wrap evidence: a caller-given integer guard in 1..H (any other value is FLM_EINVAL).  Over the parameters l < L,
 *   stats[0] = #{ |Qh| >= guard } and stats[1] = max |Qh|, both uint32, Qh = -H counting as H; stats may be NULL.
 *   L > 2^32 - 1 is FLM_ERANGE.
 *
 * flm_codec_check_modular (SA_ServiceAgent.py:538-540, 605: what the server asks before a run with the real n): FLM_EINVAL
 * for the codec's own refusals (f outside 0..30, a clip not finite and positive), pack not 2 or 4, noise_bits odd, negative
 * or above 1024, or n_clients < 1; FLM_ERANGE when one contributor's field does not fit (2 * B_n > M - 1, the packed rule
 * at n = 1) or n_clients > 2^31 - 1.  n * B_n is not bounded.  No context, no device. */
int flm_codec_check_modular(int frac_bits, float clip, int pack, int noise_bits, int64_t n_clients);
/* out[0..L) = the decode above of sum[0..ceil(L / pack)) (SA_ServiceAgent.py:538-540, 605: the final sum, as the mean of
 * `count` contributors), in the place of flm_decode_unpack_noise where the worst-case rule refuses the cohort.
 * flm_codec_check_modular's rule with n = count, then guard and L as above.  stats: two words, written, or NULL. */
int flm_decode_unpack_mod(flm_ctx *ctx, const uint32_t *sum, size_t L, int frac_bits, float clip, int pack, int noise_bits,
                          int64_t count, int guard, float *out, uint32_t *stats);
/* The same on device buffers (SA_ServiceAgent.py:538-540, 605), enqueued on `stream`; nothing is synchronised.  d_sum and
 * d_out 16-byte aligned; d_out may not overlap d_sum (FLM_EINVAL); the padding of d_out behind L is not written.  d_stats:
 * two words on the device, 4-byte aligned, zeroed on the stream first, or NULL. */
int flm_decode_unpack_mod_dev(flm_ctx *ctx, const uint32_t *d_sum, size_t L, int frac_bits, float clip, int pack,
                              int noise_bits, int64_t count, int guard, float *d_out, uint32_t *d_stats, void *stream);

/* ------------------------------ randomised block Hadamard rotation of float updates */

/* A float -> float step in front of the codec's encode and behind its decode, the flattening the
 * distributed-DP literature the codec follows applies before quantising (cpSGD; Kairouz et al., "The Distributed
 * Discrete Gaussian Mechanism", ICML 2021): the clip then has to cover about ||x||_2 / sqrt(H) per coordinate,
 * not ||x||_inf.  The rotation is linear and orthonormal, so it commutes with the secure sum and keeps the noise
 * variance per coordinate.  It stands where the reference says "For machine learning, replace it with model
 * weights" (agent/flamingo/SA_ClientAgent.py:300-304) on the way in, and behind the server's final sum
 * (SA_ServiceAgent.py:538-540, 605) on the way out.  Normative:
 *   log2_block h in 4..12, block H = 2^h parameters; a 32-byte rotation `key`, public, the same for every client and
 *     the server.  A row of L parameters is treated as L_rot = round_up(L, H) parameters; parameters >= L read as
 *     +0.0 whatever the memory behind L holds.
 *   signs: S = PRG(key), the word stream of every mask; parameter l is negated iff bit (l mod 32) of S[l / 32] is 1:
 *     indexed by parameter within the row, one sign vector for all rows of a call; a flip is an XOR of the float's
 *     sign bit.
 *   forward (client, before the encode), per block, in this order:
 *     1. an input that is NaN or +-Inf becomes +0.0 and counts as non-finite for its row (padding and parameters
 *        >= L never count);
 *     2. the sign flips;
 *     3. for s = 0, 1, ..., h - 1 in that order, for every pair (i, i ^ 2^s) with bit s of i clear:
 *        (a, b) <- (a + b, a - b), float32 round-to-nearest adds;
 *     4. every element times c_h = float32(2^(-h / 2)), once: 2^(-h / 2) exactly for even h,
 *        0x3F3504F3 * 2^(-(h - 1) / 2) for odd h;
 *     5. L_rot floats out.
 *   inverse (server, after the decode): the same butterflies in the same order on L_rot inputs, the multiply by c_h,
 *     then the sign flips; only parameters < L are written.  No non-finite handling: IEEE arithmetic on whatever
 *     comes in.
 *   Every add has fixed operands, so any evaluation order of this butterfly DAG gives the same bits.
 * Accuracy: per block |fl(y) - y| <= (h + 1) 2^-24 ||x_block||_2 per element; a quantisation error of at most
 * 2^-(f + 1) per rotated coordinate becomes at most sqrt(H) 2^-(f + 1) per original coordinate (rms unchanged).
 * The rotation is block-wise: no whole-vector transform, no padding rule but round-up-to-H, no per-client keys.
 *
 * flm_rotate_check (SA_ClientAgent.py:300-304; SA_ServiceAgent.py:538-540, 605): FLM_EINVAL for h outside 4..12 or
 * L = 0; FLM_ERANGE when the L_rot / 32 words of sign stream would pass the PRG's slot range; else *L_rot (may be
 * NULL).  No context, no device. */
int flm_rotate_check(uint64_t L, int log2_block, uint64_t *L_rot);
/* The rotation on device buffers (SA_ClientAgent.py:300-304; SA_ServiceAgent.py:538-540, 605), enqueued on `stream`;
 * nothing is synchronised.  Forward reads L and writes L_rot floats per row: x_pitch >= round_up(L, 4), out_pitch
 * >= L_rot; inverse reads L_rot and writes L: x_pitch >= L_rot, out_pitch >= round_up(L, 4).  Pitches are multiples
 * of 4, pointers 16-byte aligned.  Whatever the padding of a row holds is neither read as input nor counted, and
 * nothing behind the floats written is touched.  d_out may be d_x at equal pitches >= L_rot, in both directions.
 * d_sign_bits: ceil(L_rot / 32) words, which the caller makes with flm_prg_expand_dev(key, K = 1, L = ceil(L_rot /
 * 32), slot0 = 0); the call runs no ChaCha.  d_nonfinite (N words or NULL) is zeroed on the stream first; forward
 * only: it must be NULL for the inverse (FLM_EINVAL). */
int flm_rotate_dev(flm_ctx *ctx, const float *d_x, size_t x_pitch, int N, size_t L, int log2_block,
                   const uint32_t *d_sign_bits, int inverse, float *d_out, size_t out_pitch, uint32_t *d_nonfinite,
                   void *stream);
/* The host-pointer form (SA_ClientAgent.py:300-304; SA_ServiceAgent.py:538-540, 605): x is N x L packed and out
 * N x L_rot (forward), or N x L_rot in and N x L out (inverse); the key is expanded on the device; nonfinite: N
 * counts (written), or NULL; NULL for the inverse. */
int flm_rotate(flm_ctx *ctx, const float *x, int N, size_t L, int log2_block, const uint8_t key[32], int inverse,
               float *out, uint32_t *nonfinite);

/* ------------------------------ L2 clip of float updates, in front of the rotation */

/* The first step of the same recipe (cpSGD; Kairouz et al., above): every client scales its update to an L2 norm
 * of at most C before it rotates, rounds and adds noise.  C is the sensitivity *before* rounding: it bounds the float
 * vector, and what enters the ring is the rounded integer vector, whose norm stochastic rounding can grow by up to
 * sqrt(d) over d coordinates.  The sensitivity after rounding, the one the noise of flm_client_encode_noise_mask is
 * measured against, is Delta / 2^f of the conditional rounding below.  The codec's `clip` alone bounds
 * coordinates, which bounds the L2 norm only by clip sqrt(L).  Turning C into a privacy statement is the caller's
 * business.  It stands where the reference says "For machine learning, replace it with model weights"
 * (agent/flamingo/SA_ClientAgent.py:300-304).  Normative, per row of L float32 parameters, clip radius C (float32,
 * finite, > 0):
 *   1. squares: d_l = (double)x_l; a NaN or +-Inf input, and every parameter >= L, counts as +0.0 (the rotation's
 *      own rule: the norm is that of what the rotation transforms); d_l d_l is exact in float64.
 *   2. the sum S, in an order that depends on L only (not on N, the pitch, the grid or the stream): tiles of 4096
 *      parameters; in a tile, t = 0..255 adds the squares of parameters 16 t .. 16 t + 15 to +0.0 in index order;
 *      in each run of 64 consecutive t ("wave"), for off = 1, 2, 4, 8, 16, 32 in that order every a_t becomes
 *      a_t + a_(t ^ off) at once, after which all 64 are equal; the tile's partial is ((w0 + w1) + w2) + w3 over
 *      its four waves.  Per row, k = 0..63 adds partials k, k + 64, k + 128, ... to +0.0 in that order, and the
 *      same six steps over the 64 sums give S.  All adds are float64, round to nearest.
 *   3. the factor: s = 1.0f if S <= (double)C (double)C (exact in float64; S = 0 included), else
 *      s = (float)((double)C / sqrt(S)): IEEE double square root and division, then one rounding to float32.
 *      s <= 1; s may be a float32 subnormal for astronomically large rows (nothing is flushed to zero).
 *   4. the clip: x'_l = x_l s, one float32 round-to-nearest multiply.  A row with s == 1.0f comes out with its bits,
 *      -0.0 and subnormals included.  Standalone this is plain IEEE on whatever comes in (NaN stays NaN); fused into
 *      the forward rotation the multiply stands between the non-finite zeroing and the sign flips (steps 1 and 2
 *      of the rotation), and because a sign flip commutes exactly with a multiply, flm_rotate_clip gives the bits of
 *      flm_l2_clip followed by flm_rotate.
 * Guarantee (inputs and products normal floats): ||x'||_2 <= C (1 + 2^-22): S carries a relative error of at most
 * about L 2^-53, s one float32 rounding (2^-24), and every product one more (2^-24), which moves the norm by at most
 * that: together under 2^-22.
 *
 * flm_l2_clip_check (SA_ClientAgent.py:300-304): FLM_EINVAL for L = 0, N < 1, or C not finite and positive;
 * FLM_ERANGE when N ceil(L / 4096) passes 2^31 - 1 workgroups; else *work_doubles = N ceil(L / 4096) (may be NULL).
 * No context, no device. */
int flm_l2_clip_check(uint64_t L, float clip_norm, int N, uint64_t *work_doubles);
/* Steps 1-3 on device rows (SA_ClientAgent.py:300-304): d_factors[row] = s, and d_sumsq[row] = S unless NULL.  Two
 * launches on `stream`; nothing is synchronised.  x_pitch (floats) a multiple of 4 and >= round_up(L, 4), d_x 16-byte
 * aligned; what lies behind L in a row is never read as input.  d_work: *work_doubles doubles of the caller's,
 * written and read by this call alone, one buffer per stream in flight (the context keeps none: two streams would
 * race on it). */
int flm_l2_factors_dev(flm_ctx *ctx, const float *d_x, size_t x_pitch, int N, size_t L, float clip_norm, double *d_work,
                       float *d_factors, double *d_sumsq, void *stream);
/* Step 4 on device rows (SA_ClientAgent.py:300-304): d_out[row][l] = d_x[row][l] d_factors[row] for l < L, nothing
 * behind L written.  Pitches multiples of 4 and >= round_up(L, 4), pointers 16-byte aligned; d_out may be d_x at
 * equal pitches.  Enqueued on `stream`; nothing is synchronised. */
int flm_scale_rows_dev(flm_ctx *ctx, const float *d_x, size_t x_pitch, int N, size_t L, const float *d_factors,
                       float *d_out, size_t out_pitch, void *stream);
/* The forward rotation with step 4 in its load (SA_ClientAgent.py:300-304): flm_rotate_dev's forward arguments, rules
 * for pitches, alignment, in place and d_nonfinite, plus d_factors (N floats, from flm_l2_factors_dev on the same
 * stream or earlier).  Equals flm_scale_rows_dev followed by flm_rotate_dev bit for bit, in one pass over the row. */
int flm_rotate_clip_dev(flm_ctx *ctx, const float *d_x, size_t x_pitch, int N, size_t L, int log2_block,
                        const uint32_t *d_sign_bits, const float *d_factors, float *d_out, size_t out_pitch,
                        uint32_t *d_nonfinite, void *stream);
/* The host-pointer forms, synchronous (SA_ClientAgent.py:300-304).  flm_l2_clip: x and out N x L packed (out may be
 * x), factors N floats or NULL, sumsq N doubles or NULL: the factors, then the scale.  flm_rotate_clip: x N x L, out
 * N x L_rot, nonfinite as flm_rotate's: the factors, then the fused forward rotation under `key`. */
int flm_l2_clip(flm_ctx *ctx, const float *x, int N, size_t L, float clip_norm, float *out, float *factors, double *sumsq);
int flm_rotate_clip(flm_ctx *ctx, const float *x, int N, size_t L, int log2_block, const uint8_t key[32], float clip_norm,
                    float *out, uint32_t *nonfinite, float *factors, double *sumsq);

/* ------------------------------ conditional stochastic rounding: a bound on the rounded update's L2 norm */

/* The step between the rotation and the stochastic encode of the same recipe (Kairouz et al., above, Algorithm 1):
 * the rounding randomness is redrawn until the rounded integer vector q satisfies ||q||_2^2 <= Delta^2, so that
 * Delta / 2^f, which depends on the data through C alone, is a sensitivity the caller can hand to an accountant.
 * It stands where the reference says "For machine learning, replace it with model weights"
 * (agent/flamingo/SA_ClientAgent.py:300-304).  The pass picks the dither seed; the encode calls above then take
 * that seed unchanged, in every pack and noise mode.  Normative, per row of L float32 parameters, codec parameters
 * (f, c) and a 32-byte dither seed:
 *   q_l = int32 of the codec's stochastic encode(x_l) under that seed, r = PRG(seed)[l] indexed by parameter:
 *     exactly the integer flm_client_encode_mask rounds parameter l to, in every pack mode, before any noise;
 *   Q(seed) = sum_{l < L} q_l^2, an exact integer in uint64.  Parameters >= L and the padding of a row are never
 *     read as input.  Integer addition is associative: any order of summing gives the same bits.
 *   Of A candidate seeds the choice is the smallest a with Q(candidate a) <= max_sumsq.
 * The bound (flm_round_bound), all in float64, each operation rounded on its own, in this order:
 *   s = ((double)C * 2^f) * (1 + 2^-19); r = sqrt((double)d); b1 = (s + r) * (s + r);
 *   b2 = (s * s + (double)d * 0.25) + tail * (s + r * 0.5); *max_sumsq = (uint64)floor(min(b1, b2)).
 *   C is the L2 clip radius, d the number of coordinates encoded (L_rot behind a rotation), tail = k =
 *   sqrt(2 ln(1 / beta)) >= 0 for a per-draw failure probability of at most beta = exp(-k^2 / 2); the caller passes
 *   k, so the library calls no log.  The factor 1 + 2^-19 covers the clip's 2^-22 and the rotation's
 *   (h + 1) 2^-24 <= 13 * 2^-24.  E||q||^2 is about ||t||^2 + d / 6 while b2 carries d / 4, so few draws fail.
 *
 * flm_round_check (SA_ClientAgent.py:300-304): FLM_EINVAL for L = 0, attempts outside 1..8, and what flm_codec_check
 * refuses with n = 1 (with its code: FLM_ERANGE when ceil(c * 2^f) alone passes 2^31 - 1); FLM_ERANGE when
 * L * B^2 > 2^64 - 1, B = ceil(c * 2^f) in exact integers (Q could wrap), or ceil(L / 16) > 2^32 (the dither
 * stream's block counter).  No context, no device.
 * flm_round_bound (SA_ClientAgent.py:300-304): FLM_EINVAL for C not finite and positive, f outside 0..30, d = 0, or
 * tail negative or not finite; FLM_ERANGE for a result >= 2^63.  No context, no device. */
int flm_round_check(uint64_t L, int frac_bits, float clip, int attempts);
int flm_round_bound(float clip_norm, int frac_bits, uint64_t d, double tail, uint64_t *max_sumsq);
/* The pass on device rows (SA_ClientAgent.py:300-304): d_candidates is N x attempts x 32 bytes, candidate a of row i
 * at (i * attempts + a) * 32; d_sumsq[i * attempts + a] = Q(that candidate) (N x attempts uint64, 8-byte aligned,
 * zeroed on the stream first: the kernel adds into it); d_chosen[i] (N uint32) the choice, and d_dither[i] (N x 32
 * bytes) that candidate's bytes.  When no candidate passes d_chosen[i] = attempts and d_dither[i] holds candidate
 * 0's bytes: the row is unusable and the caller must look at d_chosen.  flm_client_encode_mask_dev's rules for d_x,
 * x_pitch and alignment.  Two launches enqueued on `stream`; nothing is synchronised, and d_dither may be handed
 * straight to flm_client_encode_*_mask_dev on the same stream.  FLM_ERANGE when N ceil(L / 4096) passes 2^31 - 1
 * workgroups; N = 0 does nothing. */
int flm_round_select_dev(flm_ctx *ctx, const float *d_x, size_t x_pitch, int N, size_t L, int frac_bits, float clip,
                         const uint8_t *d_candidates, int attempts, uint64_t max_sumsq, uint64_t *d_sumsq,
                         uint8_t *d_dither, uint32_t *d_chosen, void *stream);
/* The host-pointer form, synchronous (SA_ClientAgent.py:300-304): x N x L packed, the other arrays as above. */
int flm_round_select(flm_ctx *ctx, const float *x, int N, size_t L, int frac_bits, float clip, const uint8_t *candidates,
                     int attempts, uint64_t max_sumsq, uint64_t *sumsq, uint8_t *dither, uint32_t *chosen);

/* Device-resident PRG expansion: d_out[k*pitch + l] = PRG(seed k)[slot0 + l]. */
int flm_prg_expand_dev(flm_ctx *ctx, const uint8_t *d_seeds, int K, size_t L, uint64_t slot0,
                       uint32_t *d_out, size_t pitch, void *stream);

/* After a *_dev call has completed on its stream: number of signs that were
 * not +-1 in the last seed table (0 when valid). */
int flm_check_signs(flm_ctx *ctx, int *bad_count);

/* ----------------------------------------------------------- diagnostics */

/* Describe the launch plan the last *aggregate* call used:
 * items, tile slots, atomics used (0/1), kernel variant id (100: the one-launch
 * small-round kernel, items = its workgroups; 101: the expansion kernel of
 * flm_prg_expand[_dev], items = its one-wave workgroups). */
int flm_last_plan(const flm_ctx *ctx, int *items, int *tile_slots, int *atomics, int *variant);

/* Tuning knobs for A/B measurement (defaults are the tuned choice):
 *   "variant"  -1 auto | 0 coalesced rows | 1 block-layout rows |
 *              2 merged accumulator | 3 merged, 8 waves/SIMD budget
 *              (2/3 apply only to plans whose items each write one tile)
 *   "subtiles" 0 auto | 1 | 4 | 16 sub-tiles of 1024 slots per workgroup
 *              for aggregate plans.
 *   "pairing"  0 interleaved single-kind items | 1 dual-tile items (default) |
 *              2 same-tile window items (the window's tiles carry rows and seeds in
 *              matching parts, merged kernel), for windows where rows and masks
 *              cover different tiles.
 *   "min_items" planner target for work items per aggregate launch
 *              (default 1024; more items = finer load balance, more atomics).
 *   "ec_threads" 64 (default) | 128 | 256 lanes per workgroup of the P-256
 *              scalar-multiplication kernel.
 *   "ec_waves" 1 (default: uncapped registers) | 4 | 8 minimum waves per SIMD the
 *              scalar-multiplication kernel is compiled for (more waves, more spills).
 *   "ec_coop"  -1 (default: auto) | 0 | 1 | 2: scalar multiplications with four waves per 64 of
 *              them, the field multiplications of each point doubling and addition spread over
 *              the waves (a shorter latency chain for batches that leave most SIMDs idle); 2:
 *              the same with every field element on a 16-lane row (four products per workgroup,
 *              ~93 instructions per multiplication against ~258).
 *              Auto: the row kernel up to 20 products per CU, the cooperative kernel up to 128
 *              per CU (one pass of the device), else one lane per product.
 *   "ec_terms" 1 (default) | 2 | 4: products summed per lane in the reconstruction combine
 *              (Straus: the terms share one chain of doublings); ignored when the combine
 *              runs cooperatively.
 *   "ec_spread" 0 (default) .. 64: KiB of LDS reserved per 64-lane workgroup of the
 *              per-lane combine kernels (caps their workgroups per CU).
 *   "expand_waves" 1..256 (default 128): one-wave workgroups per CU of the expansion kernel
 *              (flm_prg_expand[_dev]), each taking a contiguous run of the K x ceil(L / 1024)
 *              seed-major (seed, 1024-slot chunk) units.
 *   "small"   0 | 1 (default) | 2: flm_aggregate_unmask_dev runs
 *              rounds as ONE small-round launch never | when rows and mask words are both
 *              <= 2^22 (BASELINE c2) | whenever the window allows it (mask_hi % 16 == 0 or
 *              mask_hi == L).  That path builds no device seed table: a following
 *              flm_aggregate_dev needs its own flm_seed_table_dev. */
int flm_set_tuning(flm_ctx *ctx, const char *key, int value);
/* The context's current value of a flm_set_tuning key (whoever set it), FLM_EINVAL for an unknown key. */
int flm_get_tuning(const flm_ctx *ctx, const char *key, int *value);

/* Host-only view of the launch planner (no GPU needed): the work items the
 * aggregate kernel would run for this round shape.  items_out receives up to
 * max_items 64-byte items (layout: flm_internal.h Item); *n_items the total;
 * *plan_flags bit0 zero-fill, bit1 atomics, bit2 single-tile, bit3 seed-light,
 * bits 8.. sub-tiles per workgroup.  subtiles/pairing as flm_set_tuning.
 * FLM_ERANGE for a mask window past 2^36 slots, by the device entry points' own rule. */
int flm_plan_aggregate(int subtiles, int pairing, size_t row_pitch, int N, int K, size_t L, size_t mask_lo,
                       size_t mask_hi, uint64_t prg_slot0, void *items_out, int max_items, int *n_items,
                       int *plan_flags);

/* ------------------------------------------------------- P-256 seed recovery */

/* Wire format: a point is 64 bytes x||y, each coordinate a 32-byte big-endian
 * integer < p (what the reference hashes, SA_ServiceAgent.py:583-585); a
 * scalar is 32 bytes big endian.  The point at infinity is returned as 64 zero
 * bytes (pycryptodome's EccPoint(0, 0)); flags bit 2 marks it.
 *
 * Threshold-ElGamal combine + key derivation, replacing
 * SA_ServiceAgent.reconstruction_process's pairwise branch (:542-585):
 *   point_i = c1_i + (negate ? -1 : +1) * sum_{j<T} lambdas[j] * shares[j][i]
 *   seed_i  = SHA-256(point_i wire bytes)          (the 32-byte ChaCha20 key)
 * for i < D, where shares[j][i] = sk_j * c0_i is committee member j's
 * decryption share (SA_ClientAgent.py:397-400) and lambdas are the Lagrange
 * coefficients at 0 (util/crypto/secretsharing points_to_secret_int).  The
 * reference computes -(sum) + c1 (negate = 1).  c1 may be NULL (base = point
 * at infinity).  shares: T*D*64 bytes, term-major; lambdas: T*32 bytes.
 * points_out (D*64), seeds_out (D*32) and flags_out (D) may each be NULL.
 * Returns FLM_EINVAL if any input point is not on P-256 (flags bit 0 = c1,
 * bit 1 = a share), as pycryptodome's EccPoint constructor raises. */
int flm_ec_combine(flm_ctx *ctx, const uint8_t *c1, const uint8_t *shares, const uint8_t *lambdas, int T, int D,
                   int negate, uint8_t *points_out, uint8_t *seeds_out, uint32_t *flags_out);
/* Device-pointer form (enqueued on `stream`; flags are written, not checked).
 * The seeds can feed flm_seed_table_dev directly, so seed recovery and the
 * unmask run back to back without a host round trip. */
int flm_ec_combine_dev(flm_ctx *ctx, const uint8_t *d_c1, const uint8_t *d_shares, const uint8_t *d_lambdas, int T,
                       int D, int negate, uint8_t *d_points_out, uint8_t *d_seeds_out, uint32_t *d_flags,
                       void *stream);
/* Shamir recovery of the self-mask seeds (SA_ServiceAgent.py:506-526):
 *   seed_i = (sum_{j<T} lambdas[j] * shares[j][i] mod n).to_bytes(32, 'big')
 * for i < M (M = |U| online clients), n = the P-256 group order (ecchash.n),
 * shares[j][i] = committee member j's decrypted share of m_i as a 32-byte
 * big-endian integer (any value < 2^256), lambdas[j] < n the Lagrange
 * coefficients at 0.  shares: T*M*32 bytes, term-major.  The seeds are the
 * ChaCha20 keys of the self masks (sign -1), ready for flm_seed_table_dev. */
/* Dropout-pair masks (SA_ServiceAgent.py:587-603) as a work queue shared by two launches on
 * different CU sets, for the CU-split reconstruction (flamingo_amd/reconstruct.py).  Units of
 * (1024 slots, 16 seeds) are claimed from d_ws[0]; every claimed unit is finished, so each unit
 * is added exactly once.
 *   final_pass = 0: d_dst[l] += sum sigma PRG(seed)[l] over the units claimed before d_ws[1]
 *                   reads non-zero (d_dst and d_ws zeroed by the caller beforehand);
 *   final_pass = 1: d_dst = d_p0 + d_p1, then the remaining units are added into d_dst.
 * groups = one-wave workgroups of the launch.  Slot l uses PRG word l (prg_slot0 = 0). */
int flm_pair_units_dev(flm_ctx *ctx, const uint8_t *d_seeds, const int8_t *d_signs, int K, const uint32_t *d_p0,
                       const uint32_t *d_p1, uint32_t *d_dst, size_t L, uint32_t *d_ws, int final_pass, int groups,
                       void *stream);
/* d_ws[1] = 1 once the work enqueued before it on `stream` has finished: the stop flag of a
 * final_pass = 0 launch running on another stream. */
int flm_flag_set_dev(flm_ctx *ctx, uint32_t *d_ws, void *stream);
int flm_shamir_combine(flm_ctx *ctx, const uint8_t *shares, const uint8_t *lambdas, int T, int M,
                       uint8_t *seeds_out);
int flm_shamir_combine_dev(flm_ctx *ctx, const uint8_t *d_shares, const uint8_t *d_lambdas, int T, int M,
                           uint8_t *d_seeds_out, void *stream);
/* Shamir dealing of the self-mask seeds, batched over M clients: replaces
 * secret_int_to_points at SA_ClientAgent.py:218-220 (the inverse of flm_shamir_combine):
 *   shares_out[c][i] = (sum_{j<T} coeffs[j][i] * xs[c]^j mod n).to_bytes(32, 'big')
 * for c < C, i < M, n the P-256 group order.  coeffs: T*M*32 bytes, term-major and big
 * endian (the layout of flm_shamir_combine's shares), term 0 the secret m_i, every value
 * < 2^256 accepted and reduced mod n (m_i is 32 random bytes).  xs: C evaluation points,
 * each non-zero (the protocol's 1..C).  shares_out: C*M*32 bytes, point-major, every value
 * < n: row c is a shares[j] of flm_shamir_combine as it stands.
 * FLM_EINVAL for T < 1, C < 1 or (host form) an x of 0; M = 0 succeeds and launches nothing.
 * _dev: device pointers (coeffs and shares 16-byte aligned, xs non-zero -- not checked),
 * enqueued on `stream`; nothing is staged or synchronised. */
int flm_shamir_deal(flm_ctx *ctx, const uint8_t *coeffs, int T, int M, const uint32_t *xs, int C,
                    uint8_t *shares_out);
int flm_shamir_deal_dev(flm_ctx *ctx, const uint8_t *d_coeffs, int T, int M, const uint32_t *d_xs, int C,
                        uint8_t *d_shares_out, void *stream);
/* AES-128-GCM with the tag dropped, n messages per call: what
 * AES.new(key, AES.MODE_GCM, nonce=nonce).encrypt(data) returns, replacing the per-share
 * encryption of SA_ClientAgent.py:227-244 (the tag is discarded at :242) and the per-share
 * decryption of :402-420 (no tag is checked, :423-425) -- so both directions are
 *   out[i] = in[i] ^ E_k(inc32(J0)) || E_k(inc32^2(J0)) || ...      (first len bytes)
 * with J0 = nonce || 0x00000001 for a 12-byte nonce and GHASH_H(nonce || 0^64 || [128]_64),
 * H = E_k(0^128), for a 16-byte one (pycryptodome's default, which the protocol uses).
 * keys: n*16 bytes; nonces: n*nonce_len, nonce_len 12 or 16; in, out: n*len, 1 <= len <= 256
 * (the protocol: 32); all dense; in == out is allowed.  FLM_EINVAL for another nonce_len or
 * len; n = 0 succeeds and launches nothing.  _dev: device pointers, enqueued on `stream`. */
int flm_aes_gcm_xor(flm_ctx *ctx, const uint8_t *keys, const uint8_t *nonces, int nonce_len, const uint8_t *in,
                    uint8_t *out, size_t len, int n);
int flm_aes_gcm_xor_dev(flm_ctx *ctx, const uint8_t *d_keys, const uint8_t *d_nonces, int nonce_len,
                        const uint8_t *d_in, uint8_t *d_out, size_t len, int n, void *stream);
/* AES-128-GCM in full (NIST SP 800-38D), n messages per call: ciphertext and 16-byte tag, what
 *   c = AES.new(key, AES.MODE_GCM, nonce=nonce); c.update(aad); ct, tag = c.encrypt_and_digest(data)
 * returns, and decrypt_and_verify on the way back.  The ciphertext is flm_aes_gcm_xor's;
 *   tag = GHASH_H(aad || 0* || ct || 0* || [8 aad_len]_64 || [8 len]_64) ^ E_k(J0).
 * keys: n*16 bytes; nonces: n*nonce_len, nonce_len 12 or 16; aad: n*aad_len, 0 <= aad_len <= 64,
 * NULL iff aad_len is 0; in, out: n*len, 0 <= len <= 256 (len 0: a tag over the AAD alone; in and
 * out are then not read and may be NULL); tags: n*16; all dense; in == out is allowed.
 * flm_aes_gcm_open recomputes each tag over the ciphertext it is given and compares all 16
 * bytes: ok_out[i] (n bytes) is 1 and out[i] the plaintext where they agree, else ok_out[i] is 0
 * and out[i] is len zero bytes -- never unauthenticated plaintext.  A wrong tag is a result, not
 * an error: the call returns 0.  FLM_EINVAL (nothing written) for another nonce_len, len or
 * aad_len, n < 0 or above 2^26, or a NULL array; n = 0 succeeds and launches nothing.
 * _dev: device pointers, enqueued on `stream` (NULL: the null stream); nothing is staged or
 * synchronised, and the call returns without waiting for earlier work on the stream. */
int flm_aes_gcm_seal(flm_ctx *ctx, const uint8_t *keys, const uint8_t *nonces, int nonce_len, const uint8_t *aad,
                     size_t aad_len, const uint8_t *in, uint8_t *out, size_t len, uint8_t *tags_out, int n);
int flm_aes_gcm_seal_dev(flm_ctx *ctx, const uint8_t *d_keys, const uint8_t *d_nonces, int nonce_len,
                         const uint8_t *d_aad, size_t aad_len, const uint8_t *d_in, uint8_t *d_out, size_t len,
                         uint8_t *d_tags_out, int n, void *stream);
int flm_aes_gcm_open(flm_ctx *ctx, const uint8_t *keys, const uint8_t *nonces, int nonce_len, const uint8_t *aad,
                     size_t aad_len, const uint8_t *in, const uint8_t *tags, uint8_t *out, size_t len,
                     uint8_t *ok_out, int n);
int flm_aes_gcm_open_dev(flm_ctx *ctx, const uint8_t *d_keys, const uint8_t *d_nonces, int nonce_len,
                         const uint8_t *d_aad, size_t aad_len, const uint8_t *d_in, const uint8_t *d_tags,
                         uint8_t *d_out, size_t len, uint8_t *d_ok_out, int n, void *stream);
/* Batched ECDSA verification on P-256, the check the reference leaves as the comment
 * `# CHECK SIGNATURES` at SA_ClientAgent.py:387: before a committee member releases its
 * decryption shares it must verify the server's signature over the offline set and the
 * members' signatures the server forwards in DEC (SA_ServiceAgent.py:382-386), or a server
 * could show different offline sets to different decryptors.  Row i: pubkeys[i] 64 wire bytes
 * x || y, digests[i] the 32-byte message digest e (any value, 0 and values >= n included; the
 * protocol's is SHA-256), sigs[i] = r || s, 2 x 32 bytes; all big endian.  The verdict is that of
 * FIPS 186-4 and OpenSSL's ECDSA_do_verify: ok_out[i] = 1 iff r, s are in [1, n-1], Q is a point
 * of the curve (not infinity), R = (e/s) G + (r/s) Q is not infinity and x(R) mod n == r; else 0.
 * flags_out (n words, may be NULL): bit 0 r or s out of range, bit 1 Q invalid (a coordinate
 * >= p, off the curve, or 64 zero bytes), bit 2 R at infinity.  An invalid signature is a
 * result, not an error: the call returns 0.  n = 0 succeeds and launches nothing; FLM_EINVAL
 * for n < 0 or n above 2^26.
 * _dev: device pointers (pubkeys, digests, sigs 16-byte aligned; d_flags may be NULL), enqueued
 * on `stream`; nothing is staged or synchronised, and the call returns without waiting for
 * earlier work on the stream. */
int flm_ecdsa_verify(flm_ctx *ctx, const uint8_t *pubkeys, const uint8_t *digests, const uint8_t *sigs, int n,
                     uint8_t *ok_out, uint32_t *flags_out);
int flm_ecdsa_verify_dev(flm_ctx *ctx, const uint8_t *d_pubkeys, const uint8_t *d_digests, const uint8_t *d_sigs,
                         int n, uint8_t *d_ok_out, uint32_t *d_flags, void *stream);
/* Batched Feldman share checks, the hot path of the committee's distributed key generation:
 * agent/dkg/SA_ClientAgent.py:219-228 (verify_commitment), which each member runs on every share
 * it receives (:150-170) and on every share broadcast after a complaint (:195-214).  Row i holds a
 * dealer d, an evaluation point x and a share s, and the check is
 *   s G == F_d(x) = sum_{k<T} x^k C_{d,k}
 * -- the reference's T scalar multiplications by the unreduced integer x ** k, here Horner's rule
 * in the exponent: T - 1 multiplications by the x_bits-bit x plus one fixed-base multiplication.
 * commitments: T*M*64 bytes, term-major (term k of dealer d at (k*M + d)*64), wire points: what
 * flm_ec_mul returns for G tiled against a flm_shamir_deal `coeffs` array.  64 zero bytes are the
 * point at infinity and a VALID commitment (a zero coefficient; the reference's EccPoint(0, 0)).
 * dealer: n indices < M, or NULL: row i then belongs to dealer i % M, so that with
 * xs[i] = x_{i / M} the rows are flm_shamir_deal's point-major shares_out as it stands.
 * xs: n values, 0 allowed (the secret against C_0); x_bits in 1..32, the number of bits of x the
 * evaluation walks, the same for every row; shares: n*32 bytes, big endian.
 * ok_out[i] (n bytes) = 1 iff the share is < n (the group order), every commitment of the row's
 * dealer is infinity or a point of the curve, x < 2^x_bits and s G = F_d(x); else 0.
 * flags_out (n words, may be NULL): bit 0 share >= n, bit 1 a commitment with a coordinate >= p
 * or off the curve (it counts as infinity in F), bit 2 F_d(x) at infinity, bit 3 x >= 2^x_bits
 * (F is then evaluated at x mod 2^x_bits).  points_out (n*64, may be NULL): the affine wire form
 * of F_d(x), a member's public verification key material; infinity as 64 zero bytes.  The verdict
 * never depends on points_out.  A failed check is a result, not an error: the call returns 0.
 * FLM_EINVAL, with nothing written, for T < 1, M < 1, x_bits outside 1..32, n < 0, n or T*M
 * above 2^26, a NULL commitments, xs, shares or ok_out, or (host form only) a dealer index >= M;
 * n = 0 succeeds and launches nothing.
 * _dev: device pointers (commitments, shares and points_out 16-byte aligned), enqueued on
 * `stream` (NULL: the null stream); nothing is staged or synchronised, and the call returns
 * without waiting for earlier work on the stream.  A dealer index >= M is NOT checked there: the
 * kernel would read outside `commitments`. */
int flm_feldman_verify(flm_ctx *ctx, const uint8_t *commitments, int T, int M, const uint32_t *dealer,
                       const uint32_t *xs, int x_bits, const uint8_t *shares, int n, uint8_t *ok_out,
                       uint8_t *points_out, uint32_t *flags_out);
int flm_feldman_verify_dev(flm_ctx *ctx, const uint8_t *d_commitments, int T, int M, const uint32_t *d_dealer,
                           const uint32_t *d_xs, int x_bits, const uint8_t *d_shares, int n, uint8_t *d_ok_out,
                           uint8_t *d_points_out, uint32_t *d_flags, void *stream);
/* Batched scalar multiplication out[i] = scalars[i] * points[i]: the ECDH
 * (SA_ClientAgent.py:256-263), ElGamal (:434-447) and decryption-share
 * (:397-400) products, n independent elements per call. */
int flm_ec_mul(flm_ctx *ctx, const uint8_t *points, const uint8_t *scalars, int n, uint8_t *out, uint32_t *flags_out);
/* Hash to curve, replacing util/crypto/ecchash.hash_str_to_curve (:277-283) as the client calls
 * it for its pairwise seed group element (SA_ClientAgent.py:283-286): expand_message_xmd with
 * SHA-256 and DST "QUUX-V01-CS02-with-P256_XMD:SHA-256_SSWU_RO_" to 96 bytes (:90-133), two field
 * elements OS2IP(48 bytes) mod n (the client passes the group order as the modulus, :285;
 * hash_to_field :50-61), the reference's map_to_curve of each (:233-275), and their sum (:282).
 * flm_hash_to_curve: msgs n x 64 bytes, message i in its first lens[i] <= 64 bytes.
 * flm_hash_to_curve_decimal: the messages are str(v) for v in [v0, v0 + n) -- the client's h_ijt is
 * str(x & 0xFFFF) (:280), so v0 = 0, n = 65536 is every value it can hash: one launch.
 * out: n x 64 wire bytes; flags bit 2: the sum is the point at infinity (out zeros); FLM_EINVAL if
 * a map found no square root (flags bit 3; not expected).  _dev: device buffers, enqueued on
 * `stream`, flags written but not checked.  Square roots are a^((p+1)/4): libnum's sqrtmod root
 * order is assumed to yield that root first (the one convention not pinned by the reference). */
int flm_hash_to_curve(flm_ctx *ctx, const uint8_t *msgs, const uint32_t *lens, int n, uint8_t *out,
                      uint32_t *flags_out);
int flm_hash_to_curve_decimal(flm_ctx *ctx, uint32_t v0, int n, uint8_t *out, uint32_t *flags_out);
int flm_hash_to_curve_decimal_dev(flm_ctx *ctx, uint32_t v0, int n, uint8_t *d_out, uint32_t *d_flags, void *stream);

/* ------------------------------------------------ CU-partitioned streams */

/* A HIP stream whose kernels run only on the CUs set in `mask` (n_words
 * 32-bit words, bit i = logical CU i; hipExtStreamCreateWithCUMask).  The
 * server reconstruction (SA_ServiceAgent.py:499-605) runs its latency-bound
 * EC combine on a few CUs of one such stream while the VALU-bound self-mask
 * unmask fills the complementary set on another, so neither evicts the other's
 * workgroups.  *n_cus receives the device's CU count. */
int flm_cu_count(flm_ctx *ctx, int *n_cus);
int flm_stream_create_cu_mask(flm_ctx *ctx, const uint32_t *mask, int n_words, void **stream_out);
int flm_stream_destroy(flm_ctx *ctx, void *stream);

/* ------------------------------------------------ multi-GPU (RCCL over xGMI) */

/* The round shards two ways over G GPUs: rank r ingests clients
 * [N*r/G, N*(r+1)/G) and sums them over all L slots, regenerates every seed's
 * mask over its own slot shard [lo_r, hi_r) only, and ONE reduce-scatter of the
 * partial vectors (ncclUint32, ncclSum -- mod 2^32, so every ring order gives
 * the same bits) returns rank r the slots [lo_r, hi_r) of the reference's
 * final_sum = vec_sum_partial + cancel_vec + mi_vec (SA_ServiceAgent.py:346-350,
 * 529-605).  Shards are S = round_up(L, 1024*G) / G slots (the partial vectors
 * are S*G long); trailing ranks may own an empty shard. */
int flm_shard_bounds(size_t L, int n_ranks, int rank, size_t *lo, size_t *hi, size_t *shard_words);
int flm_client_bounds(int N, int n_ranks, int rank, int *c0, int *c1);

/* One process per GPU: rank 0 makes a 128-byte RCCL unique id, every rank
 * passes it to flm_comm_init_rank (collective: all ranks must call it), and the
 * context then owns the communicator (released by flm_free).
 * flm_reduce_scatter_dev: d_recv[0..recv_words) = rank's slice of the elementwise
 * uint32 sum over ranks of d_send[0..recv_words*n_ranks).  flm_all_gather_dev:
 * byte all-gather (d_recv = n_ranks * send_bytes), e.g. recovered pair seeds.
 * stream NULL = the HIP null stream, as for every *_dev call.  flm_comm_size
 * returns 1 when no communicator is attached (then *n_ranks = 1, *rank = 0).
 * flm_rccl_available: 1 when RCCL could be loaded (dlopen) and every symbol
 * resolved, else 0 (reason in flm_last_error(NULL)); local, not collective, so
 * every rank can agree on it before any rank enters flm_comm_init_rank.
 * flm_comm_destroy: synchronise the context's device, then ncclCommFinalize + ncclCommDestroy
 * the attached communicator (no-op without one); the context stays usable.  Call it on every
 * rank BEFORE the process's other RCCL users (torch.distributed's nccl process group) are torn
 * down -- the teardown order of distributed.shutdown -- so no library communicator is left for
 * an exit-time destructor. */
int flm_rccl_available(void);
int flm_comm_destroy(flm_ctx *ctx);
int flm_comm_unique_id(uint8_t id_out[128]);
int flm_comm_init_rank(flm_ctx *ctx, int n_ranks, int rank, const uint8_t id[128]);
int flm_comm_size(flm_ctx *ctx, int *n_ranks, int *rank);
int flm_reduce_scatter_dev(flm_ctx *ctx, const uint32_t *d_send, uint32_t *d_recv, size_t recv_words, void *stream);
int flm_all_gather_dev(flm_ctx *ctx, const void *d_send, void *d_recv, size_t send_bytes, void *stream);

/* One process, G GPUs -- the drop-in server's form: the reference server is a
 * single-threaded DES process (Kernel.py:190-271), so the group owns one
 * context per device and an RCCL clique (ncclCommInitAll).  devices: G device
 * ids, all distinct (RCCL) or all equal (loopback: the ranks share one GPU and
 * exchange through a device kernel instead of RCCL -- tests and rehearsal on a
 * one-GPU box); NULL = 0..G-1.  G <= 16.
 * flm_group_aggregate_unmask: flm_aggregate_unmask over every device: host
 * rows in (one host thread per device uploads that device's clients), out (L
 * words, host) back; synchronous.
 * flm_group_aggregate_unmask_dev: rows already resident (d_rows[r]: n_rows[r]
 * rows at row_pitch on device r; d_seeds[r]/d_signs[r] on device r); enqueues
 * every rank's round and the exchange on the ranks' context streams and
 * returns; d_shards[r] (>= S words on device r) receives slots [lo_r, hi_r).
 * The rounds run on the ranks' context streams (flm_ctx_stream(flm_group_ctx(g, r))):
 * the caller orders them after the work that produced the inputs.  A group of
 * one device needs no RCCL: its round writes the shard (the whole vector) directly.
 * flm_group_sync waits for every rank's stream.
 * flm_group_init_flags(..., FLM_GROUP_RCCL): give the group an RCCL clique even
 * when it has one device (ncclCommInitAll(1, {dev})); its rounds then take the
 * multi-GPU path -- partial buffer, grouped ncclReduceScatter, shard -- so the code
 * the 8-GPU node runs is exercised on a one-GPU box.  Refused for loopback groups
 * (RCCL does not allow two ranks on one GPU).  flm_group_has_rccl: 1 when the group
 * has a clique. */
typedef struct flm_group flm_group;
#define FLM_GROUP_RCCL 1u
int flm_group_init(flm_group **out, int n, const int *devices);
int flm_group_init_flags(flm_group **out, int n, const int *devices, unsigned flags);
int flm_group_has_rccl(const flm_group *g);
void flm_group_free(flm_group *g);
const char *flm_group_last_error(const flm_group *g);
int flm_group_size(const flm_group *g);
int flm_group_is_loopback(const flm_group *g);
flm_ctx *flm_group_ctx(flm_group *g, int rank);
int flm_group_sync(flm_group *g);
int flm_group_aggregate_unmask(flm_group *g, const uint32_t *const *rows, int N, const uint8_t *seeds,
                               const int8_t *signs, int K, size_t L, uint32_t *out);
int flm_group_aggregate_unmask_dev(flm_group *g, const uint32_t *const *d_rows, size_t row_pitch, const int *n_rows,
                                   const uint8_t *const *d_seeds, const int8_t *const *d_signs, int K, size_t L,
                                   uint32_t *const *d_shards);

/* ------------------------------------------- device-resident VECTOR ingestion */

/* The server's VECTOR bodies on the GPU(s) from arrival to the final sum: the reference keeps
 * each body in a dict on arrival (SA_ServiceAgent.py:205-210), sums them in report_process
 * (:346-350) and adds the recovered masks in reconstruction_process (:529-540, :587-605).
 * flm_store_create: on one context (ctx) or across a group (g; exactly one of them), L slots,
 *   `capacity` rows expected (the store grows past it).
 * flm_store_add: copies row[0..n) into pinned staging and returns; the DMA onto the sender's
 *   device row runs on a copy stream of the store (rows round-robin over the group's devices in
 *   arrival order; a sender that sends twice overwrites its row, like the reference's dict).
 *   n != L is remembered and makes flm_store_partial fail with the reference's message (:348-349).
 * flm_store_partial: enqueues S = sum of the stored rows after their uploads; S stays on the
 *   device(s) (slot-sharded on a group, after the group's one reduce-scatter).  Returns at once;
 *   flm_store_partial_wait blocks until S is complete and gives the device time in ms.
 * flm_store_partial_host: S to the host (inspection only; the round never needs it there).
 * flm_store_unmask: out[0..L) = S + sum_k signs[k] * PRG(seeds[k]), each device over its own
 *   slot shard (no exchange), then the one copy to the host; synchronous.
 * flm_store_reset: forget the rows (the next arrivals wait for the last partial sum's reads). */
typedef struct flm_store flm_store;
int flm_store_create(flm_store **out, flm_ctx *ctx, flm_group *g, size_t L, int capacity);
void flm_store_free(flm_store *st);
const char *flm_store_last_error(const flm_store *st);
int flm_store_count(const flm_store *st);
int flm_store_add(flm_store *st, int64_t sender, const uint32_t *row, size_t n);
int flm_store_partial(flm_store *st);
int flm_store_partial_wait(flm_store *st, float *gpu_ms);
int flm_store_partial_host(flm_store *st, uint32_t *out);
int flm_store_unmask(flm_store *st, const uint8_t *seeds, const int8_t *signs, int K, uint32_t *out);
/* flm_store_unmask with each device's slot shard decoded in place (flm_decode_sum_dev) before its copy to the
 * host: out[0..L) = decode(final sum, count), the mean of `count` contributors as float32
 * (SA_ServiceAgent.py:538-540, 605 and the codec above; SA_ClientAgent.py:300-324 made the input). */
int flm_store_unmask_f32(flm_store *st, const uint8_t *seeds, const int8_t *signs, int K, int frac_bits,
                         int64_t count, float *out);
/* flm_store_unmask of a store of packed rows (SA_ServiceAgent.py:538-540, 605 and the packed codec above;
 * SA_ClientAgent.py:300-324 made the input): the store's length must be ceil(L_params / pack), else
 * FLM_EINVAL.  Each device decodes its word shard [lo, hi) into the floats [pack * lo, min(pack * hi,
 * L_params)) of a float buffer of its own (flm_decode_unpack_dev) before its copy to the host:
 * out[0..L_params) is the mean of `count` contributors.  The packed headroom rule with n = count. */
int flm_store_unmask_unpack_f32(flm_store *st, const uint8_t *seeds, const int8_t *signs, int K, size_t L_params,
                                int frac_bits, float clip, int pack, int64_t count, float *out);
/* flm_store_unmask_unpack_f32 of noised packed rows (SA_ClientAgent.py:300-324 and
 * agent/examples/crypto/PPFL_ClientAgent.py:219-221, 274-285 made the input): the bias is
 * count * (B + noise_bits / 2); the noised headroom rule with n = count.  noise_bits = 0 is
 * flm_store_unmask_unpack_f32. */
int flm_store_unmask_unpack_noise_f32(flm_store *st, const uint8_t *seeds, const int8_t *signs, int K,
                                      size_t L_params, int frac_bits, float clip, int pack, int noise_bits,
                                      int64_t count, float *out);
/* flm_store_unmask_unpack_noise_f32 with the decode modulo the field (SA_ServiceAgent.py:538-540, 605 and "decode modulo
 * the field" above; SA_ClientAgent.py:300-324 made the input): each device decodes its word shard with
 * flm_decode_unpack_mod_dev, a word's cascade never leaving the word; the host adds the devices' near counts and takes
 * the maximum of their maxima into stats (two words, or NULL).  flm_decode_unpack_mod's rules with n = count. */
int flm_store_unmask_unpack_mod_f32(flm_store *st, const uint8_t *seeds, const int8_t *signs, int K, size_t L_params,
                                    int frac_bits, float clip, int pack, int noise_bits, int64_t count, int guard,
                                    float *out, uint32_t *stats);
/* Device time (ms, rank 0's stream) of the last flm_store_unmask, from its seed upload to the end of
 * its copy of final_sum to the host: the part of the call's wall time the GPU accounts for. */
int flm_store_unmask_ms(const flm_store *st, float *gpu_ms);
int flm_store_reset(flm_store *st);

/* Allocate / free page-locked host memory through HIP (for a pinned arena
 * holding client vectors, so host->device copies are DMA at full PCIe rate). */
void *flm_host_alloc(size_t bytes);
void flm_host_free(void *p);

#ifdef __cplusplus
}
#endif

#endif /* FLAMINGO_HIP_H */
