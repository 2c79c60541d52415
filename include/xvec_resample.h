/* xvec_resample.h -- C ABI of waveform resampling in libxvec_hip.so: band-limited sinc interpolation at any ratio.
 *
 * The first arithmetic stage of the reference's Dataset.__getitem__ (dataset.py:125-130): wavfile.read -> resampy.resample ->
 * cut_to_sec -> augment_data -> min/max -> mfcc.  The reference calls the resampler on every file and every MUSAN clip, also at
 * equal rates, where the signal still passes through the filter's low-pass: identity at equal rates is NOT what it computes.
 * With one ratio per row the same kernel does speed perturbation (ratio 1 / factor).
 *
 * The arithmetic is resampy 0.3.0's resample_f, RESTATED (resampy is not installed where this was written: parity with the
 * package is unpinned, tests/resample_ref.py holds the restatement the kernel is checked against).  The filter is half of a
 * windowed sinc, win[nwin] fp64 with P = 2 ** precision entries per zero crossing (nwin = P * num_zeros + 1).  For a row of len
 * samples at ratio = sr_new / sr_orig:
 *   n_out = int(len * ratio);  inc = 1.0 / ratio;  scale = min(1.0, ratio);  step = int(scale * P)        (step is TRUNCATED)
 *   win_s[j] = win[j] * ratio if ratio < 1 else win[j]
 *   for t in 0 .. n_out - 1:
 *     time = t * inc;  n0 = int(time);  frac = scale * (time - n0);  idx = frac * P;  off = int(idx);  eta = idx - off
 *     for i in 0 .. min(n0 + 1, (nwin - off) / step) - 1:         j = off + i * step          (left wing, i ascending)
 *       acc = acc + (win_s[j] + eta * (win_s[j + 1] - win_s[j])) * x[n0 - i]
 *     frac = scale - frac;  idx = frac * P;  off = int(idx);  eta = idx - off
 *     for k in 0 .. min(len - n0 - 1, (nwin - off) / step) - 1:   j = off + k * step          (then the right wing, k ascending)
 *       acc = acc + (win_s[j] + eta * (win_s[j + 1] - win_s[j])) * x[n0 + k + 1]
 * with win_s[nwin] read as win_s[nwin - 1] (the package's delta[nwin - 1] = 0).  Every operation is fp64 and rounded on its own:
 * no fused multiply-add anywhere.  XVEC_RESAMPLE_ACC_F64 keeps acc in fp64 (the package with float64 input);
 * XVEC_RESAMPLE_ACC_F32 rounds acc to fp32 after every tap (the package with int16 or float32 input, whose output array is
 * float32).  The result is converted ONCE to the output dtype.  An output is therefore a pure function of its row, its ratio and
 * the table: bit-identical from run to run, whatever the batch, the strides, the base alignment or the tile it falls into, and
 * identical for an int16 input and the same values as fp32.  A truncated step (512 / 3 -> 170) widens the filter when
 * downsampling: a 1 kHz sine taken from 48 kHz to 16 kHz is 2.7e-3 off the analytic sine (3e-8 when upsampling).  That is the
 * package's behaviour at that version and is kept.
 *
 * Conventions as xvec_augment.h: DEVICE pointers unless a parameter says HOST, asynchronous on the caller's stream, no allocation
 * (the caller passes a workspace of the queried size, whose previous contents never matter), return codes as xvec_hip.h (0 = OK)
 * with the message from xvec_resample_last_error().  No float atomics.  Argument errors (null pointers, sizes < 1, a ratio that is
 * not finite or not positive, step < 1, a row stride smaller than its row, out_cols smaller than the longest output, a workspace
 * that is too small) return XVEC_ERR_ARG / XVEC_ERR_TOO_LARGE / XVEC_ERR_WORKSPACE before the device is touched.
 */
#ifndef XVEC_RESAMPLE_H
#define XVEC_RESAMPLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xvec_stream; /* hipStream_t */

#define XVEC_RESAMPLE_X_F32 0
#define XVEC_RESAMPLE_X_I16 1
#define XVEC_RESAMPLE_OUT_F32 0
#define XVEC_RESAMPLE_OUT_F64 1
#define XVEC_RESAMPLE_ACC_F32 0
#define XVEC_RESAMPLE_ACC_F64 1
#define XVEC_RESAMPLE_LEN_I64 0
#define XVEC_RESAMPLE_LEN_I32 1
/* A block of XVEC_RESAMPLE_TILE threads owns XVEC_RESAMPLE_TILE consecutive outputs of one row, a lane per output.  Where the
 * input samples a tile can touch (xvec_resample_tile_span) number at most XVEC_RESAMPLE_SPAN_MAX, the block stages them in LDS
 * as fp32 (32 KiB); at a smaller ratio the lanes read the row from memory.  Both give the same bits. */
#define XVEC_RESAMPLE_TILE 256
#define XVEC_RESAMPLE_SPAN_MAX 8192
#define XVEC_RESAMPLE_PRECISION_MAX 20

const char* xvec_resample_last_error(void);

/* int(n * ratio): the outputs of a row of n samples, so that callers can size `out`.  -1 for n < 0 or a ratio that is not
 * finite and positive. */
int64_t xvec_resample_out_len(int64_t n, double ratio);

/* floor((XVEC_RESAMPLE_TILE - 1) / ratio) + 1 + 2 * (nwin / step): the input samples one tile can touch at this ratio.
 * -1 for arguments xvec_resample would refuse. */
int64_t xvec_resample_tile_span(double ratio, int64_t nwin, int32_t precision);

/* Scratch of xvec_resample (0 for sizes the call would refuse): the per-row ratio plans. */
size_t xvec_resample_workspace_bytes(int32_t batch, int32_t n_ratios);

/* x [batch, n] fp32 or int16 (x_dtype), row stride ld_in >= n elements.  lens [batch] int64 or int32 (len_dtype), the valid
 * samples of every row, or NULL for n everywhere; an entry outside 0 .. n is clamped into it, samples past it are never read.
 * ratios: HOST array [n_ratios], n_ratios == 1 (one ratio for every row) or == batch (row b at ratios[b]).
 * win [nwin] fp64, the UNSCALED table, nwin >= 2 ** precision + 1, 0 <= precision <= XVEC_RESAMPLE_PRECISION_MAX.
 * out [batch, out_cols] fp32 or fp64 (out_dtype), row stride ld_out >= out_cols; out_cols >= int(n * ratio) of every row.
 * Columns >= n_out_b of row b are written as 0 (all of them where n_out_b == 0).  out_len [batch] (len_dtype) receives n_out_b.
 * 1 <= batch, n, out_cols, nwin <= 2^31 - 1.  out must not overlap x. */
int xvec_resample(const void* x, int32_t x_dtype, int64_t ld_in, int32_t batch, int64_t n, const void* lens, int32_t len_dtype,
                  const double* ratios, int32_t n_ratios, const double* win, int64_t nwin, int32_t precision, int32_t acc_mode,
                  void* out, int32_t out_dtype, int64_t ld_out, int64_t out_cols, void* out_len, void* workspace,
                  size_t workspace_bytes, xvec_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* XVEC_RESAMPLE_H */
