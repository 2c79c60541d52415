/* xvec_diar.h -- C ABI of speaker diarization's clustering step in libxvec_hip.so: agglomerative hierarchical clustering with
 * average linkage of the window-by-window score matrices of a batch of recordings.
 *
 * The reference has no diarization; this is the step the x-vector diarization recipe (Kaldi's callhome recipe) puts behind the
 * scorer, as identification is the step a recognition system puts there.  The oracle is scipy.cluster.hierarchy.linkage with
 * method 'average' on the negated scores (tests/test_diarize.py, through the numpy restatement tests/diar_ref.py).
 *
 * Input.  S is fp64, row-major with row stride ld.  Recording r owns the diagonal block of rows and columns rec_start[r] ..
 * rec_start[r + 1] - 1, n_r of them.  Only cells with row < column inside a block are ever read: the diagonal, the lower triangle
 * and everything outside the blocks may hold anything, NaN included.  S is not modified; the working copy (symmetric, dense, one
 * matrix per recording) lives in the workspace.
 *
 * Algorithm: greedy average linkage (UPGMA) on similarities.  Every segment starts as a cluster of size 1, named by its index
 * within the recording.  A step takes the pair of live clusters (i, j), i < j, with the largest score; ties go to the lowest i,
 * then the lowest j; NaN is never selected; -0.0 == +0.0 and +-inf are ordinary values.  The merged cluster keeps the name i
 * and the size n_i + n_j, and for every other live k
 *   s_ik = (n_i * s_ik + n_j * s_jk) / (n_i + n_j)
 * with the sizes as doubles: two products, one sum, one division, each rounded on its own, nothing contracted.  The merge list
 * is therefore a pure function of the block: bit-identical from run to run and whatever ld, the base alignment (8 bytes is all
 * that is asked), the other recordings, n_rec or the recording's place in the batch are.
 *
 * Stop rule, before every step, with c live clusters and `best` the score of the pair that would merge.  Stop when there is no
 * selectable pair (c == 1, or every remaining pair is NaN).  Otherwise, if want_host != NULL and want_host[r] > 0: merge iff
 * c > want_host[r]; else merge iff best >= threshold or (max_clusters > 0 and c > max_clusters).  threshold = +inf never merges
 * by score, -inf merges everything; want_host[r] > n_r merges nothing.
 *
 * Output.  labels[rec_start[r] + s] is the cluster of segment s of recording r, clusters numbered 0 .. n_clusters[r] - 1 in the
 * order of their lowest segment index (a canonical labelling: two runs compare element by element).  With the merge outputs,
 * recording r owns slots rec_start[r] .. rec_start[r + 1] - 2 of the three arrays: (i, j, score at the merge) in merge order;
 * the slots of merges that were not performed, and each recording's last slot, hold -1, -1, NaN.
 *
 * One block per recording, persistent over its merges: XVEC_DIAR_THREADS_SMALL threads (a single wave) for n_r <=
 * XVEC_DIAR_THREADS_SMALL, XVEC_DIAR_THREADS_LARGE beyond; a row whose cached best partner was merged away is rescanned by one
 * wave, XVEC_DIAR_RESCAN_WIDTH cells at a time.  Every loop has a trip count fixed by n_r at launch, no block waits on another.
 *
 * Conventions as xvec_hip.h: DEVICE pointers (but rec_start_host and want_host: HOST arrays, checked there and copied into the
 * workspace on the stream -- when the call is captured into a graph, they are read again at every replay), asynchronous on the
 * caller's stream, no allocation (the caller passes a workspace of the queried size), return codes as xvec_hip.h (0 = OK) with
 * the message from xvec_diar_last_error().  No float atomics.
 */
#ifndef XVEC_DIAR_H
#define XVEC_DIAR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xvec_stream; /* hipStream_t */

/* segments (windows) of one recording, at most: the block keeps a row's best partner, size and label in LDS (24 bytes a row) */
#define XVEC_DIAR_MAX_SEGMENTS 2048
/* threads of the block of a recording with n_r <= XVEC_DIAR_THREADS_SMALL segments (one wave), and of every larger one */
#define XVEC_DIAR_THREADS_SMALL 64
#define XVEC_DIAR_THREADS_LARGE 256
/* cells of a row one wave reads at a time when it rescans the row (a lane each) */
#define XVEC_DIAR_RESCAN_WIDTH 64

const char* xvec_diar_last_error(void);

/* Bytes of workspace for xvec_ahc_cluster on these recordings (0 for arguments that are refused). */
size_t xvec_ahc_workspace_bytes(const int64_t* rec_start_host, int32_t n_rec);

/* rec_start_host: n_rec + 1 HOST offsets from 0, every recording with 1 .. XVEC_DIAR_MAX_SEGMENTS segments, fewer than 2^31 in
 * all; ld >= rec_start_host[n_rec].  want_host [n_rec] (HOST) may be NULL.  labels [N] and n_clusters [n_rec] int32;
 * merge_i / merge_j [N] int32 and merge_score [N] fp64: all three NULL, or none.  A NaN threshold, a negative max_clusters
 * and a negative want_host[r] are refused. */
int xvec_ahc_cluster(const double* S, int64_t ld, const int64_t* rec_start_host, int32_t n_rec, double threshold,
                     int32_t max_clusters, const int32_t* want_host, int32_t* labels, int32_t* n_clusters, int32_t* merge_i,
                     int32_t* merge_j, double* merge_score, void* workspace, size_t workspace_bytes, xvec_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* XVEC_DIAR_H */
