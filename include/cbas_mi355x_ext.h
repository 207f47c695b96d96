/* cbas_mi355x_ext.h - the extension surface of libcbas_mi355x.so.
 *
 * The core C ABI (cbas_mi355x.h, CBAS_ABI_VERSION) is closed: its entry points, their number and their version stay as they
 * are.  What is added beside it is declared here, carries the prefix cbasx_ and is exported by both builds of the library
 * (csrc/exports.map).  The error model is the core's: a non-zero return is a CBAS_E* code of cbas_mi355x.h and
 * cbas_last_error() holds the message of the calling thread.
 *
 * Sequence decoding (csrc/seq_viterbi.hip): the most likely label sequence of every clip under a
 * first-order transition model, from per-frame probabilities that are already on the device.
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

#ifdef __cplusplus
}
#endif

#endif /* CBAS_MI355X_EXT_H */
