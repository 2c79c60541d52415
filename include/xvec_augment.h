/* xvec_augment.h -- C ABI of waveform augmentation in libxvec_hip.so: SNR mixing, reverberation, min-max scaling.
 *
 * The stage in front of the MFCC front end, as the reference's Dataset.augment_data runs it (dataset.py:185-396):
 *   mix        add_with_certain_snr over the MUSAN kinds (music, speech, noise): noise added at a drawn SNR
 *   reverb     augment_rir: the signal plus its convolution with a room impulse response, peak-matched
 *   normalize  dataset.py:217-219: (x - min) / max(x - min), applied to every sample, augmented or not
 * All randomness stays on the host: the device does arithmetic on the draws it is handed (which clip, which start,
 * which SNR).  Resampling (resampy) is the unit in front of this one (xvec_resample.h); file reading is not part of the library.
 *
 * Conventions as xvec_eval.h: DEVICE pointers unless a parameter says HOST, asynchronous on the caller's stream, no
 * allocation (the caller passes a workspace of the queried size), return codes as xvec_hip.h (0 = OK) with the message
 * from xvec_aug_last_error().  No float atomics, every reduction in a fixed order (sums of squares are integer sums,
 * maxima are order-independent): repeat calls on the same inputs give bit-identical outputs.  The workspace's previous
 * contents never matter.
 *
 * Argument errors (null pointers, sizes < 1, an op whose slice leaves its row or whose source range leaves the source
 * list, ops not sorted by utterance, a workspace that is too small) return XVEC_ERR_ARG / XVEC_ERR_WORKSPACE before the
 * device is touched.  What only the device can see is handled in the kernel and counted in xvec_aug_status: a source
 * whose pool row is outside the pool (or whose start is negative) contributes zeros, an utterance whose rir index is
 * >= n_rirs (or whose rir_len is outside 1 .. l_max) is left alone; neither is ever dereferenced.
 *
 * Degenerate inputs follow the reference, which divides by zero there: an all-zero utterance or impulse response in
 * xvec_aug_reverb and a constant row in xvec_aug_normalize give NaN in that row (0 / 0), without a fault.  An all-zero
 * noise in xvec_aug_mix is not degenerate (the 1e-20 in the divisor): the gain is finite and the output is trunc(x).
 */
#ifndef XVEC_AUGMENT_H
#define XVEC_AUGMENT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* xvec_stream; /* hipStream_t */

#define XVEC_AUG_POOL_F32 0
#define XVEC_AUG_POOL_I16 1

/* One add_with_certain_snr over waves[utt, offset : offset + length].  Its noise z is the sum, in list order, of the
 * sources srcs[first_src .. first_src + n_src): z[i] = sum pool[row, start + i], zeros past the clip's end (the pad of
 * cut_to_sec).  snr_ratio = 10 ** (snr_db / 10), computed by the host. */
typedef struct {
    int32_t utt;
    int32_t offset;
    int32_t length;
    int32_t first_src;
    int32_t n_src;
    int32_t reserved;      /* 0 */
    double snr_ratio;
} xvec_aug_op;

typedef struct {
    int32_t row;           /* pool row */
    int32_t start;         /* first sample of the clip that is used */
} xvec_aug_src;

/* Written by the device: xvec_aug_mix sets n_bad_source, xvec_aug_reverb sets n_bad_rir, each leaves the other alone. */
typedef struct {
    int64_t n_bad_source;  /* (op, source) pairs skipped */
    int64_t n_bad_rir;     /* utterances left alone because their rir index or its length was out of range */
} xvec_aug_status;

const char* xvec_aug_last_error(void);

/* Scratch of xvec_aug_mix (0 for sizes the call would refuse): the fp64 working signal [batch, n] and the op list. */
size_t xvec_aug_mix_workspace_bytes(int32_t batch, int64_t n, int64_t n_ops);

/* waves fp32 [batch, n], row stride ld >= n, in place.  pool [n_rows, m_max] fp32 or int16 (pool_dtype) with the clip
 * lengths src_len[n_rows].  ops: HOST array [n_ops], sorted by utt (n_ops may be 0: nothing happens); srcs [n_srcs].
 *
 * The ops of one utterance run in list order, each on the result of the one before, on an fp64 copy of the row that is
 * rounded to fp32 once at the end; a row without ops is not touched.  One op, with x the slice of the working signal:
 *   s = trunc(x), zt = trunc(z)                      (toward zero: the reference's astype('int64'))
 *   s_rms = sqrt(sum s^2 / length), z_rms = sqrt(sum zt^2 / length)     (64-bit integer sums: exact, order-independent)
 *   w = sqrt(s_rms * s_rms / snr_ratio),  out = s + (zt * w) / (z_rms + 1e-20)      (fp64, in this order)
 * gains_out [n_ops] fp64 receives w / (z_rms + 1e-20) of every op. */
int xvec_aug_mix(float* waves, int64_t ld, int32_t batch, int64_t n, const void* pool, int32_t pool_dtype, int32_t n_rows,
                 int64_t m_max, const int32_t* src_len, const xvec_aug_op* ops, int64_t n_ops, const xvec_aug_src* srcs,
                 int64_t n_srcs, double* gains_out, xvec_aug_status* status, void* workspace, size_t workspace_bytes,
                 xvec_stream stream);

/* Scratch of xvec_aug_reverb: the first n outputs of every convolution and the block maxima. */
size_t xvec_aug_reverb_workspace_bytes(int32_t batch, int64_t n, int64_t l_max);

/* waves fp32 [batch, n], row stride ld, in place.  rirs fp32 [n_rirs, l_max] with rir_len[n_rirs]; rir_of_utt[batch],
 * a negative entry leaves the row alone (bit for bit).  Per utterance, with h its response of L taps:
 *   c = x * h (full convolution, n + L - 1 outputs),  out = x + c[:n] * (max|x| / max|c|)
 * max|c| runs over all n + L - 1 outputs.  The convolution is a Toeplitz product on the fp32 matrix pipe
 * (v_mfma_f32_32x32x2_f32): every output is an fp32 sum of L exact products.  n <= 2^28, l_max <= 2^24. */
int xvec_aug_reverb(float* waves, int64_t ld, int32_t batch, int64_t n, const float* rirs, int32_t n_rirs, int64_t l_max,
                    const int32_t* rir_len, const int32_t* rir_of_utt, xvec_aug_status* status, void* workspace,
                    size_t workspace_bytes, xvec_stream stream);

/* Every row of waves fp32 [batch, n] (row stride ld), in place: (x - min) / (max - min) in fp32; the row's minimum maps
 * to exactly 0 and its maximum to exactly 1. */
int xvec_aug_normalize(float* waves, int64_t ld, int32_t batch, int64_t n, xvec_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* XVEC_AUGMENT_H */
