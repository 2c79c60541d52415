/* xvec_der.h -- C ABI of diarization's scoring step in libxvec_hip.so: the diarization error rate (DER) of hypothesis turns
 * against reference turns, with the one-to-one speaker mapping that maximises the matched time.
 *
 * The definition follows NIST md-eval's (miss, false alarm and speaker confusion, overlapped speech on both sides, a
 * no-score collar, the optimal mapping), but neither md-eval nor dscore nor pyannote.metrics is a dependency: the text below
 * is the specification, the oracle is its numpy restatement (tests/der_ref.py, the optimum of the mapping from scipy's
 * linear_sum_assignment); parity with md-eval, dscore and pyannote.metrics is UNPINNED.
 *
 * Time axis.  Time is integer ticks.  Recording r owns ticks 0 .. n_r - 1 with n_r = rec_start_host[r + 1] - rec_start_host[r];
 * rec_start_host is a HOST int64 [n_rec + 1] that starts at 0, every recording has at least 1 tick, the total stays below 2^31.
 *
 * Turns.  A turn list is a DEVICE int32 [m, 4] array, row-major, of (rec, start, end, spk): the turn covers ticks
 * start .. end - 1.  m = 0 is allowed, with a NULL pointer.  A turn is INVALID if rec is outside 0 .. n_rec - 1, spk is outside
 * 0 .. XVEC_DER_MAX_SPEAKERS - 1, or end <= start.  Invalid turns are ignored and counted: ignored is int64 [2], reference then
 * hypothesis.  A valid turn is clipped to its recording.  Turns of one side may overlap each other in any way: a tick carries
 * a speaker SET per side, R_t and H_t, each a 64-bit mask.
 *
 * Scored ticks.  With collar >= 0 in ticks, the unscored ticks of recording r are those t with b - collar <= t < b + collar,
 * intersected with the recording, for b every start and every end of every valid REFERENCE turn, taken as given (before the
 * clipping; touching turns of one speaker are not merged).  With skip_overlap != 0, ticks with popcount(R_t) > 1 are unscored
 * too.  Everything below sums over scored ticks only.
 *
 * Counts per recording, all int64, with Nref = popcount(R_t) and Nhyp = popcount(H_t):
 *   scored = the number of scored ticks;  total = sum Nref;  miss = sum max(0, Nref - Nhyp);  fa = sum max(0, Nhyp - Nref);
 *   C[i][j] = the number of scored ticks with i in R_t and j in H_t, 64 x 64;
 *   the mapping: a partial injective map from reference to hypothesis speakers that maximises correct = sum_i C[i][map(i)];
 *   conf = sum min(Nref, Nhyp) - correct;
 *   der[r] = (miss + fa + conf) / total, one fp64 division of the two int64 values each converted to fp64, NaN when total == 0;
 *   der[n_rec] pools the batch: the summed errors over the summed totals (NaN when that is 0).
 *
 * Mapping output.  map is int32 [n_rec, 64]: map[r][i] is the hypothesis speaker of reference speaker i, or -1.  A pair with
 * C[i][j] == 0 is never reported (it comes back as -1).  Where several maps reach the optimum, which one comes back is not
 * specified, but it is a pure function of the recording's C: bit-identical from run to run, alone or in a batch, at any place
 * in the batch.  Everything is integer arithmetic, so every count is exact; there are no float atomics.
 *
 * Kernels.  Four launches and one memset per xvec_der_score, whatever n_rec and the turn counts are: (1) a wave per turn ORs
 * its speaker bit into the per-tick masks and, for a reference turn, its two collar zones into the no-score bitmap; (2) a
 * block per XVEC_DER_CHUNK_TICKS consecutive ticks of one recording, each of its waves walking XVEC_DER_WAVE_ROWS rows of 64
 * consecutive ticks with a lane per tick: along a row, the first lane of every run of one pair (R_t, H_t) adds the run's
 * length to the block's 64 x 64 LDS histogram and the other lanes of the run add nothing; (3) a wave per recording with a lane per hypothesis speaker solves the assignment by shortest augmenting
 * paths on int64 potentials, ties to the lowest lane; (4) one block pools the batch.  EVERY loop of the solver has a trip count
 * of at most 64 fixed at launch, whatever the data; no block waits on another.
 *
 * Conventions as xvec_diar.h: DEVICE pointers (but rec_start_host: a HOST array, checked there, copied into the workspace on
 * the stream and read again at every replay of a captured graph), asynchronous on the caller's stream, no allocation (the
 * caller passes a workspace of the queried size), return codes as xvec_hip.h (0 = OK) with the message from
 * xvec_der_last_error().
 */
#ifndef XVEC_DER_H
#define XVEC_DER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xvec_stream; /* hipStream_t */

/* speakers of one side in one recording at most: a bit of the tick's mask, a lane of the solver's wave each */
#define XVEC_DER_MAX_SPEAKERS 64
/* consecutive ticks of one recording that one block of the counting pass owns */
#define XVEC_DER_CHUNK_TICKS 4096
/* rows of 64 consecutive ticks that one wave of that block walks, a lane per tick */
#define XVEC_DER_WAVE_ROWS 16
/* threads of a block */
#define XVEC_DER_THREADS 256

const char* xvec_der_last_error(void);

/* Bytes of workspace for xvec_der_cooccurrence / xvec_der_score on these recordings (0 for arguments that are refused). */
size_t xvec_der_workspace_bytes(const int64_t* rec_start_host, int32_t n_rec, int64_t m_ref, int64_t m_hyp);

/* Turns -> counts [n_rec, 4] int64 (scored, total, miss, fa), cooc [n_rec, 64, 64] int64, ignored [2] int64. */
int xvec_der_cooccurrence(const int32_t* ref_turns, int64_t m_ref, const int32_t* hyp_turns, int64_t m_hyp,
                          const int64_t* rec_start_host, int32_t n_rec, int32_t collar, int32_t skip_overlap, int64_t* counts,
                          int64_t* cooc, int64_t* ignored, void* workspace, size_t workspace_bytes, xvec_stream stream);

/* The optimal mapping of a batch of 64 x 64 int64 matrices cooc [n_rec, 64, 64]: map [n_rec, 64] int32 and correct [n_rec]
 * int64.  Entries must lie in 0 .. 2^31 - 1; the kernel does not check them: for an entry outside the range that recording's
 * result is unspecified, the kernel still terminates and touches no other recording.  One launch, no workspace. */
int xvec_der_assign(const int64_t* cooc, int32_t n_rec, int32_t* map, int64_t* correct, xvec_stream stream);

/* The fused call: counts [n_rec, 5] int64 (scored, total, miss, fa, conf), map [n_rec, 64] int32, der [n_rec + 1] fp64,
 * ignored [2] int64, and cooc [n_rec, 64, 64] int64, which may be NULL.  Nothing crosses to the host in between. */
int xvec_der_score(const int32_t* ref_turns, int64_t m_ref, const int32_t* hyp_turns, int64_t m_hyp,
                   const int64_t* rec_start_host, int32_t n_rec, int32_t collar, int32_t skip_overlap, int64_t* counts,
                   int32_t* map, double* der, int64_t* ignored, int64_t* cooc, void* workspace, size_t workspace_bytes,
                   xvec_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* XVEC_DER_H */
