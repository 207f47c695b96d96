/* cbas_mi355x_ext.h - the extension surface of libcbas_mi355x.so.
 *
 * The core C ABI (cbas_mi355x.h, CBAS_ABI_VERSION) is closed: its entry points, their number and their version stay as they
 * are.  What is added beside it is declared here, carries the prefix cbasx_ and is exported by both builds of the library
 * (csrc/exports.map).  The error model is the core's: a non-zero return is a CBAS_E* code of cbas_mi355x.h and
 * cbas_last_error() holds the message of the calling thread.
 *
 * Sequence decoding (csrc/seq_viterbi.hip): the most likely label sequence of every clip under a
 * first-order transition model, from per-frame probabilities that are already on the device.
 * Forward-backward (csrc/seq_hmm.hip): the posterior probabilities of every frame under the same model,
 * the expected transition counts and the log-likelihood.
 */
#ifndef CBAS_MI355X_EXT_H
#define CBAS_MI355X_EXT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Scores are integers: CBASX_VITERBI_UNIT units per factor of two, so a probability p scores 256 * log2(p).  Integer
 * addition and maximum are associative, which is what lets a long clip be decoded piecewise and still give the serial
 * definition bit for bit. */
#define CBASX_VITERBI_UNIT 256
#define CBASX_VITERBI_SCORE_MIN (-8192)          /* the score of p <= 2^-32, of a negative p and of a NaN */
#define CBASX_VITERBI_TRANS_LIMIT (1 << 20)      /* transitions and priors lie in [-2^20, 2^20] */
#define CBASX_VITERBI_MAX_CLASSES 64
/* Frames one workgroup walks.  A clip of more frames is cut into pieces of this many and decoded by as many workgroups
 * (DESIGN.md section 24 says why 1024: a piece's back-pointers, 1024 * C bytes, fit the LDS for C = 64, and the chunk walk
 * along a 2 000 000-frame clip has about as many steps as the frame walk inside one piece). */
#define CBASX_VITERBI_CHUNK 1024
#define CBASX_VITERBI_FLAG_NAN 1u                /* *flags_dev of cbasx_viterbi_scores: a probability was a NaN */

/* scores_dev (n_total, C) int32 from probs_dev (n_total, C) float32:
 *     e = clamp((int32) rintf(256 * log2f(max(p, 2^-32))), -8192, 0)
 * (an exact power of two scores exactly 256 * its exponent).  A NaN or a negative p gives -8192; a NaN also ORs
 * CBASX_VITERBI_FLAG_NAN into *flags_dev, which the caller zeroes.  One streaming pass, asynchronous on `stream`; nothing
 * is copied.  1 <= C <= 64, n_total >= 0. */
int cbasx_viterbi_scores(const float* probs_dev, int64_t n_total, int32_t C, int32_t* scores_dev, uint32_t* flags_dev,
                         void* stream);

/* Bytes of workspace cbasx_viterbi_decode needs for this shape, or -1 for a shape it refuses (n_total < 0, n_clips < 1,
 * C outside 1 .. 64, more than 2^31 - 1 pieces). */
int64_t cbasx_viterbi_workspace_bytes(int64_t n_total, int32_t n_clips, int32_t C);

/* labels_dev (n_total) int32: per clip of clip_table_dev (n_clips, 2) int64 = (first frame, frames) the Viterbi path
 *     d_0[j] = prior[j] + e_0[j]
 *     d_t[j] = max_i (d_{t-1}[i] + A[i][j]) + e_t[j],   bp_t[j] = the lowest i that attains the maximum
 *     end    = the lowest j that attains max_j d_{T-1}[j];  the labels follow the back-pointers from it
 * with A[i][j] = log_trans_dev[i * C + j] (from state i to state j), prior = log_prior_dev (NULL: zeros) and e = scores_dev
 * (n_total, C) int32 in [-8192, 0].  clip_score_dev (n_clips) int64, when not NULL, gets that final maximum, exact; a clip
 * of 0 frames gets 0 and writes no label.  Frames outside every clip get -1.  Clips must not overlap (the caller's rule, as
 * for cbas_labels_median); every table entry is checked before it is used.  A clip of more than CBASX_VITERBI_CHUNK frames is
 * decoded piecewise by several workgroups; the result is that of the serial definition, and a clip's labels depend neither
 * on the other clips of the call nor on where the clip lies.
 *
 * Refusals (CBAS_EINVAL): a NULL pointer other than log_prior_dev / clip_score_dev; C outside 1 .. 64; n_total < 0;
 * n_clips < 1; a workspace smaller than cbasx_viterbi_workspace_bytes or not 256-byte aligned; a table entry that reaches
 * outside n_total; a transition or prior outside [-2^20, 2^20]; a score outside [-8192, 0].  The last three are found by one
 * checking pass on the device that writes only into the workspace; the call SYNCHRONISES `stream` ONCE to read its verdict
 * and queues the decoding kernels - the first that write labels_dev / clip_score_dev - only after it.  So a refused call
 * leaves both outputs untouched, and an accepted call returns with the decoding queued, not finished. */
int cbasx_viterbi_decode(const int32_t* scores_dev, int64_t n_total, const int64_t* clip_table_dev, int32_t n_clips, int32_t C,
                         const int32_t* log_trans_dev, const int32_t* log_prior_dev, int32_t* labels_dev,
                         int64_t* clip_score_dev, void* workspace_dev, int64_t workspace_bytes, void* stream);

/* Forward-backward (csrc/seq_hmm.hip): the sum half of the same model.  Transitions and prior are
 * float32 PROBABILITIES here, not integer scores: every entry finite and at least 0, every row (and the prior) summing to 1
 * within CBASX_HMM_ROW_TOL. */
#define CBASX_HMM_MAX_CLASSES 64
/* Frames one wave walks; a clip of more frames is cut into pieces of this many, relative to its own first frame, as
 * cbasx_viterbi_decode cuts it (the walk along the pieces of a 2 000 000-frame clip has about as many
 * steps as the frame walk inside one piece). */
#define CBASX_HMM_CHUNK 1024
#define CBASX_HMM_FLOOR_LOG2 (-32)               /* an emission is max(p, 2^-32) */
#define CBASX_HMM_ROW_TOL 1e-4f
#define CBASX_HMM_FLAG_EMISSION 1u               /* *flags_dev: a probability of a clip's frame was a NaN or negative */
#define CBASX_HMM_FLAG_POSTERIOR 2u              /* *flags_dev: alpha o beta of a frame summed to 0 or not finitely; its row is NaN */

/* Bytes of workspace cbasx_hmm_posteriors needs for this shape, or -1 for a shape it refuses (n_total < 0, n_clips < 1,
 * C outside 1 .. 64, more than 2^31 - 1 pieces).  With K = n_total / 1024 + n_clips and KT = 2 * (n_total / 1024) + 1, every
 * part rounded up to 256 bytes: 256 + 2 * 4 n_clips + 2 * 8 (n_clips + 1) + KT * (4 C^2 + 12 C) + K * (8 C^2 + 8). */
int64_t cbasx_hmm_workspace_bytes(int64_t n_total, int32_t n_clips, int32_t C);

/* gamma_dev (n_total, C) float32: per clip of clip_table_dev (n_clips, 2) int64 = (first frame, frames), with frames
 * 0 .. T-1, emissions b_t[j] = max(p_t[j], 2^-32) from probs_dev (n_total, C) float32, A[i][j] = trans_dev[i * C + j] (from
 * state i to state j) and prior = prior_dev (NULL: 1 / C),
 *     a_0 = prior o b_0,  a_t = (alpha_{t-1} A) o b_t,  alpha_t = a_t / sum(a_t),  loglik = sum_t log2 sum(a_t)
 *     beta_{T-1} = 1,     beta_t ~ A (b_{t+1} o beta_{t+1})
 *     gamma_t = alpha_t o beta_t / its sum
 *     xi_t[i][j] = alpha_t[i] A[i][j] b_{t+1}[j] beta_{t+1}[j] / its sum over i, j
 * gamma_t is P(state_t | the whole clip).  When not NULL, xi_dev (C, C) float64 gets the sum of xi_t over all clips and
 * t < T-1, pi_dev (C) float64 the sum of gamma_0 over all clips, loglik_dev (n_clips) float64 every clip's log-likelihood in
 * bits.  Frames outside every clip get a gamma row of zeros; a clip of 0 frames contributes nothing and has loglik 0.  alpha
 * and beta run in float64 and are kept in range by powers of two only, never by each other's sums.  A NaN or negative
 * probability inside a clip counts as 2^-32 and ORs CBASX_HMM_FLAG_EMISSION into *flags_dev; a frame whose alpha o beta sums to 0 or not finitely gets
 * a row of NaN, counts nothing in xi and ORs CBASX_HMM_FLAG_POSTERIOR.  The caller zeroes *flags_dev.  gamma_dev must not
 * overlap probs_dev: it holds alpha between the two passes, so no (n_total, C) workspace is needed.  Clips must not overlap.
 *
 * A clip of more than CBASX_HMM_CHUNK frames is cut into pieces and walked by several waves; the sums are added per clip in
 * ascending piece order and then in ascending clip order in float64, without atomics, so two calls agree bit for bit and a
 * clip's gamma and loglik depend neither on the other clips of the call nor on where the clip lies.  gamma does not depend
 * on which of xi_dev / pi_dev / loglik_dev are NULL.
 *
 * Refusals (CBAS_EINVAL): a NULL pointer other than prior_dev / xi_dev / pi_dev / loglik_dev; C outside 1 .. 64; n_total < 0;
 * n_clips < 1; a workspace smaller than cbasx_hmm_workspace_bytes or not 256-byte aligned; a table entry that reaches outside
 * n_total; a transition row or a prior that is not finite, negative or off 1 by more than 1e-4.  The last three are found
 * by one checking pass on the device that writes only into the workspace; the call SYNCHRONISES `stream` ONCE to read its
 * verdict, exactly as cbasx_viterbi_decode does, and queues the kernels that write the outputs only after it.  So a refused
 * call leaves gamma_dev, xi_dev, pi_dev and loglik_dev untouched, and an accepted call returns with the work queued. */
int cbasx_hmm_posteriors(const float* probs_dev, int64_t n_total, const int64_t* clip_table_dev, int32_t n_clips, int32_t C,
                         const float* trans_dev, const float* prior_dev, float* gamma_dev, double* xi_dev, double* pi_dev,
                         double* loglik_dev, uint32_t* flags_dev, void* workspace_dev, int64_t workspace_bytes, void* stream);

/* The motif HMM's two passes over resident rows (csrc/rows_hmm.hip).  rows_f16_dev is (n_rows, dim) fp16 with
 * row stride ld, as cbas_rows_kmeans_* takes it: dim a multiple of 32 up to 1536, ld >= dim and a multiple of 8, 16-byte aligned.
 * The working row u of a row x is x widened to fp32 (normalize = 0) or fl(x * rn) with rn = fp32(1 / sqrt(s)), s the fp32 sum of
 * squares in the order s = (l0 + l1) + (l2 + l3), l_j the fmaf chain over the columns d with (d % 32) / 8 = j, ascending - the rn
 * of cbas_rows_search and cbas_rows_kmeans_*; a zero row has rn = 0.  The rows are finite. */
#define CBASX_ROWS_HMM_MAX_STATES 64
#define CBASX_ROWS_HMM_MAX_DIM 1536
#define CBASX_ROWS_HMM_MAX_PARTS 256             /* cbasx_rows_weighted_sums deals the rows to at most this many parts ... */
#define CBASX_ROWS_HMM_PART_ROWS 64              /* ... of a multiple of this many rows each */

/* probs_dev (n_rows, C) float32, the emission probabilities of every row under C mean directions means_dev (C, dim) float32
 * with one shared concentration kappa (von Mises-Fisher emissions of equal kappa, whose normaliser cancels):
 *     z_j = fmaf(kappa, fl(rn * (x . mu_j)), logw_j)       (rn = 1 with normalize = 0; logw = log_weights_dev, NULL: zeros)
 *     probs_j = exp(z_j - max z) / sum_j exp(z_j - max z)
 *     lognorm = (max z + log sum_j exp(z_j - max z)) * log2(e)
 * lognorm_dev (n_rows) float32, when not NULL, is that log-normaliser in bits, the unit of cbasx_hmm_posteriors' loglik.
 * Sum orders: x . mu_j = chain0 + chain1, chain p the fp32 fmaf chain, from 0, over the columns d with (d / 32) % 2 = p ordered by
 * (d / 32, d % 8, (d % 32) / 8) ascending (cbas_rows_search's dot); the sum over j adds, for f = 0 .. 15, the states f, 16 + f,
 * 32 + f, 48 + f in ascending order and then the 16 results by the pairwise tree of strides 1, 2, 4, 8; the division is
 * correctly rounded.  A zero row (rn = 0) and kappa = 0 give exactly the softmax of logw.  A row's outputs depend neither on
 * n_rows, nor on the grid, nor on where the row lies; two calls agree bit for bit.  One streaming pass, asynchronous on `stream`;
 * nothing is copied, no atomics.
 * A mean or a log-weight that is not finite is the caller's error: the probs and lognorm of the rows it meets are unspecified
 * (NaN included; a log-weight of -infinity alone simply gives its state probability 0); nothing else is written.
 * Refusals (CBAS_EINVAL, the outputs untouched): a NULL pointer other than log_weights_dev / lognorm_dev; C outside 1 .. 64; dim or
 * ld out of range; n_rows < 0; normalize not 0 or 1; kappa negative or not finite; rows or means not 16-byte aligned. */
int cbasx_rows_emissions(const void* rows_f16_dev, int64_t n_rows, int32_t dim, int64_t ld, int32_t C, int32_t normalize,
                         const float* means_dev, float kappa, const float* log_weights_dev, float* probs_dev, float* lognorm_dev,
                         void* stream);

/* Bytes of workspace cbasx_rows_weighted_sums needs, or -1 for a shape it refuses.  With rpp = max(64, ceil(ceil(n_rows / 256) /
 * 64) * 64) rows per part and parts = ceil(n_rows / rpp) <= 256 - functions of n_rows alone -: max(parts, 1) * (4 C dim + 256)
 * bytes, every piece rounded up to 16: never more than 256 * (4 C dim + 256), however many rows. */
int64_t cbasx_rows_weighted_sums_workspace_bytes(int64_t n_rows, int32_t dim, int32_t C);

/* The M step: sums_dev (C, dim) float64 = sum_t w[t][c] u_t and mass_dev (C) float64 = sum_t w[t][c], from weights_dev
 * (n_rows, C) float32 (the gamma of cbasx_hmm_posteriors).  The product runs on the fp32 matrix pipe straight from the fp16 rows;
 * u = fl(x * rn) is formed between the load and the MFMA operand.
 * Sum order: part p owns the rows p rpp .. (p + 1) rpp - 1.  Inside a part the 16-row blocks go to four lanes in turn (block b to
 * lane b % 4); a lane is ONE fp32 fused-multiply-add chain per (state, column), from 0, over its rows in ascending order; the
 * part's value is ((lane 0 + lane 1) + lane 2) + lane 3 in fp32; the parts are added in ascending order in float64.  mass is the
 * same chain with u = 1.  No atomics: two calls agree bit for bit.  A row whose weights are all 0 contributes nothing (frames
 * outside every clip are such rows in gamma); a NaN weight propagates into its state's sums and mass.  n_rows = 0 gives zeros.
 * Asynchronous on `stream`; nothing is copied.
 * Refusals (CBAS_EINVAL, the outputs untouched): a NULL pointer; C outside 1 .. 64; dim or ld out of range; n_rows < 0; normalize
 * not 0 or 1; a workspace smaller than cbasx_rows_weighted_sums_workspace_bytes or not 16-byte aligned; rows not 16-byte aligned;
 * sums or mass not 8-byte aligned. */
int cbasx_rows_weighted_sums(const void* rows_f16_dev, int64_t n_rows, int32_t dim, int64_t ld, int32_t C, int32_t normalize,
                             const float* weights_dev, double* sums_dev, double* mass_dev, void* workspace_dev,
                             int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CBAS_MI355X_EXT_H */
