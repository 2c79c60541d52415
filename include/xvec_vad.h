/* xvec_vad.h -- C ABI of the two steps between the MFCC front end and the extractor in libxvec_hip.so: energy-based voice
 * activity detection and sliding-window cepstral mean (and variance) normalisation, with the selection of the voiced frames.
 *
 * The reference has neither; they are the steps every Kaldi-style x-vector recipe puts there (compute-vad-decision,
 * apply-cmvn-sliding, select-voiced-frames).  The definitions below are Kaldi's ComputeVadEnergy and SlidingWindowCmn RESTATED
 * from memory: neither Kaldi nor a port of it is installed where this was written, so parity with Kaldi is UNPINNED, and this
 * header is the specification.  tests/vad_ref.py restates it in numpy; the kernels are checked against that.
 *
 * Input.  x is fp32 [B, T, C]: frame t of utterance b starts at x + b * utt_stride + t * row_stride (strides in floats,
 * row_stride >= C, utt_stride >= (T - 1) * row_stride + C).  lengths is int32 [B], each in 0 .. T (values outside are clamped
 * to that range); NULL means T frames everywhere.  A frame at or past its utterance's length, and the floats between a row's C
 * values and the next row, are never read for their value: they may hold NaN.
 *
 * Energy VAD (xvec_vad_options), for an utterance of L frames with e[t] = x[t, energy_col] (column 0 is c0, which the MFCC
 * front end writes as the log frame energy):
 *   thr    = energy_threshold + energy_mean_scale * (S / L)      S = the sum of (double)e[t], t < L, in the order below; fp64,
 *            every operation rounded on its own, nothing contracted.  With energy_mean_scale == 0, thr = energy_threshold and S
 *            is not formed.  With a mean scale an empty utterance has thr = 0 / 0 = NaN.
 *   hot[t] = (double)e[t] > thr                                   strict; a NaN e[t] is never hot, a NaN thr makes nothing hot
 *   num(t) = the hot frames among t' = max(0, t - frames_context) .. min(L - 1, t + frames_context); den(t) = that many frames
 *   voiced[t] = (double)num >= (double)den * proportion_threshold                                   (one fp64 product)
 * The order of S: XVEC_VAD_LANES partial sums, partial j adding e[j], e[j + XVEC_VAD_LANES], ... in ascending order from 0.0;
 * then for stride = XVEC_VAD_LANES / 2, / 4, ..., 1: partial[j] += partial[j + stride] for j < stride; S = partial[0].  The order
 * depends on L alone, so the decisions are a pure function of the utterance's own frames: bit-identical whatever B, the strides
 * and the utterance's place in the batch are.
 * Outputs: mask uint8 [B, T] with row stride mask_stride >= T (1 = voiced; entries at or past the length are 0), counts int32
 * [B] (the voiced frames), thr fp64 [B] (optional).
 *
 * Sliding CMVN (xvec_cmvn_options).  The window [lo, hi) of frame t in an utterance of L frames (integer arithmetic):
 *   center:  lo = t - cmn_window / 2;  hi = lo + cmn_window
 *   else:    lo = t - cmn_window;      hi = t + 1
 *   if lo < 0:  hi -= lo; lo = 0
 *   if !center and hi > t:  hi = max(t + 1, min_window)
 *   if hi > L:  lo -= hi - L; hi = L; if lo < 0: lo = 0
 * so that 0 <= lo <= t < hi <= L and n = hi - lo <= max(cmn_window + 1, min_window).  Per channel c:
 *   mean = (the fp64 sum of x[t', c], t' = lo .. hi - 1, in the order below) / n
 *   y    = (float)((double)x[t, c] - mean)
 * and with norm_vars: y = 0 if n == 1, else var = sumsq / n - mean * mean (the squares formed and summed in fp64, in the same
 * order), floored at 1e-10, and y = (float)(((double)x[t, c] - mean) * var^-0.5), var^-0.5 as 1.0 / sqrt(var).
 * The order of the window sums.  The frames of an utterance are cut into tiles of F frames from its first frame, and a tile
 * into runs of R frames from the tile's first frame; F, the channels G of a group and R = ceil(F / min(F, max(1,
 * XVEC_VAD_LANES / G))) follow from C and the options alone (csrc/vad_plan.h).  The first frame of a run adds its window's
 * values (and squares) to 0.0 in ascending order; every following frame of the run first adds the values that enter its
 * window, ascending, then subtracts those that leave it, ascending.  An output is therefore a pure function of its
 * utterance's frames and the options: bit-identical from run to run and whatever B, T, the strides, the other utterances, the
 * mask and the utterance's place in the batch are.  Against sums formed afresh for every frame the values differ within the
 * fp64 summation error of the run (tests/vad_ref.py bounds it): they are held to that bound, not to bits.
 *
 * Select.  With a mask, row r of utterance b of y is the normalised row of the utterance's r-th voiced frame (a mask entry
 * counts as voiced when it is nonzero AND lies below the length); new_lengths[b] is their number, and rows new_lengths[b] ..
 * T - 1 are written as zeros: the extractor's ragged calls take a zero-padded batch.  Without a mask y has the input's layout,
 * rows at or past the length are zeros and new_lengths[b] (optional then) is the length.  With options == NULL the rows are
 * not normalised: bit-exact copies.  y must not overlap x.
 *
 * Kernels.  Decide: one block of XVEC_VAD_LANES threads per utterance (the sum, the votes, the mask, the count, and the
 * voiced frames in front of every chunk of XVEC_VAD_LANES frames).  Normalise-and-select: a block per (utterance, tile of
 * frames, group of channels) stages the tile's rows and its window halo in LDS as fp32; the plan (csrc/vad_plan.h) picks the
 * tile height (XVEC_CMVN_TILE_MAX halving down to XVEC_CMVN_TILE_MIN) and the channel group so that the rows fit
 * XVEC_CMVN_LDS_BYTES.  xvec_vad_cmvn is those two launches; xvec_cmvn_sliding with a mask first counts the mask's chunks
 * (two launches), without one it is a single launch; xvec_vad_energy is one.  xvec_vad_cmvn gives the same bits as
 * xvec_vad_energy followed by xvec_cmvn_sliding with that mask.
 *
 * Conventions as xvec_diar.h: DEVICE pointers, asynchronous on the caller's stream, graph-capturable, no allocation (the
 * caller passes a workspace of the queried size, whose previous contents never matter), every loop's trip count fixed at
 * launch, no block waits on another, no float atomics.  Return codes as xvec_hip.h (0 = OK) with the message from
 * xvec_vad_last_error().  Argument errors return XVEC_ERR_ARG (a small workspace XVEC_ERR_WORKSPACE) before the device is touched.
 */
#ifndef XVEC_VAD_H
#define XVEC_VAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xvec_stream; /* hipStream_t */

/* partial sums of the energy sum, threads of the decide kernel's block, frames of a chunk whose leading count it writes */
#define XVEC_VAD_LANES 256
/* channels of a frame, at most */
#define XVEC_VAD_MAX_CHANNELS 1024
/* cmn_window at most; min_window at most XVEC_CMVN_MAX_WINDOW + 1 */
#define XVEC_CMVN_MAX_WINDOW 1900
/* frames of a tile: the largest power of two in this range whose rows fit the LDS budget */
#define XVEC_CMVN_TILE_MAX 256
#define XVEC_CMVN_TILE_MIN 16
/* channels of a group never go below this (or C) when the plan splits the channels: 32 contiguous bytes a row */
#define XVEC_CMVN_GROUP_MIN 8
/* LDS for the staged rows of one block (beside them the block keeps 1 KiB of output rows): 60 KiB, two blocks a CU */
#define XVEC_CMVN_LDS_BYTES 61440

typedef struct xvec_vad_options {
    double energy_threshold;     /* 5.0 */
    double energy_mean_scale;    /* 0.5 */
    double proportion_threshold; /* 0.6; strictly between 0 and 1 */
    int32_t frames_context;      /* 0; >= 0 */
    int32_t energy_col;          /* 0; 0 .. C - 1 */
} xvec_vad_options;

typedef struct xvec_cmvn_options {
    int32_t cmn_window; /* 600; 1 .. XVEC_CMVN_MAX_WINDOW */
    int32_t min_window; /* 100; 1 .. XVEC_CMVN_MAX_WINDOW + 1; only read when center == 0 */
    int32_t center;     /* 0 */
    int32_t norm_vars;  /* 0 */
} xvec_cmvn_options;

const char* xvec_vad_last_error(void);

/* Bytes of workspace for xvec_cmvn_sliding and xvec_vad_cmvn on a batch of B utterances of T frames (0 for B or T below 1). */
size_t xvec_vad_workspace_bytes(int32_t B, int32_t T);

/* The decisions alone.  thr may be NULL. */
int xvec_vad_energy(const float* x, int32_t B, int32_t T, int32_t C, int64_t row_stride, int64_t utt_stride,
                    const int32_t* lengths, const xvec_vad_options* vad, uint8_t* mask, int64_t mask_stride, int32_t* counts,
                    double* thr, xvec_stream stream);

/* Normalise (cmvn != NULL) and select (mask != NULL).  y is fp32 [B, T, C] with strides of its own under the rules of x's.
 * new_lengths may be NULL without a mask.  The workspace may be NULL without a mask. */
int xvec_cmvn_sliding(const float* x, int32_t B, int32_t T, int32_t C, int64_t row_stride, int64_t utt_stride,
                      const int32_t* lengths, const xvec_cmvn_options* cmvn, const uint8_t* mask, int64_t mask_stride, float* y,
                      int64_t y_row_stride, int64_t y_utt_stride, int32_t* new_lengths, void* workspace, size_t workspace_bytes,
                      xvec_stream stream);

/* Decide, then normalise (cmvn != NULL) and, with select != 0, keep the voiced frames; with select == 0 y has the input's
 * layout and new_lengths (may be NULL then) the lengths, while mask and counts still hold the decisions.  thr may be NULL. */
int xvec_vad_cmvn(const float* x, int32_t B, int32_t T, int32_t C, int64_t row_stride, int64_t utt_stride, const int32_t* lengths,
                  const xvec_vad_options* vad, const xvec_cmvn_options* cmvn, int32_t select, uint8_t* mask, int64_t mask_stride,
                  int32_t* counts, double* thr, float* y, int64_t y_row_stride, int64_t y_utt_stride, int32_t* new_lengths,
                  void* workspace, size_t workspace_bytes, xvec_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* XVEC_VAD_H */
