// The class-sum column walk of the statistics kernels: what xvec_plda_stats (plda_train.hip), xvec_lda_stats (lda.hip) and
// xvec_model_mean (ident.hip) share.  Included INSIDE the including file's anonymous namespace (class_scatter.h does it for the
// first two), after <algorithm> and host_support.h.  With the class_start checks and upload of their host sides.
#pragma once

// rows [b, e) of `order` that class c owns, clamped to [0, n]
__device__ __forceinline__ void class_rows(const int64_t* __restrict__ cstart, int c, int64_t n, int64_t& b, int64_t& e) {
    b = std::min<int64_t>(std::max<int64_t>(cstart[c], 0), n);
    e = std::min<int64_t>(std::max<int64_t>(cstart[c + 1], b), n);
}

// The column walk of a class-sum kernel, one block per class c: sums[c, d] = sum of x[order[i], d] over i in [b, e), a column
// per thread (four interleaved partial sums per column, combined in a fixed order).  `order` must be a permutation of 0 .. n-1 (the
// ABI cannot check a device array): an index outside [0, n) is only kept from reading out of bounds -- it adds nothing, and
// the outputs are undefined.  x has row stride ld >= dim, sums is dense.
template <typename T>
__device__ __forceinline__ void class_sum_columns(const T* __restrict__ x, int64_t n, int dim, int64_t ld,
                                                  const int* __restrict__ order, int c, int64_t b, int64_t e,
                                                  double* __restrict__ sums) {
    auto at = [&](int r, int d) -> double { return (r >= 0 && r < n) ? (double)x[(int64_t)r * ld + d] : 0.0; };
    for (int d = threadIdx.x; d < dim; d += 256) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        int64_t i = b;
        for (; i + 4 <= e; i += 4) {
            const int r0 = order[i], r1 = order[i + 1], r2 = order[i + 2], r3 = order[i + 3];
            a0 += at(r0, d);
            a1 += at(r1, d);
            a2 += at(r2, d);
            a3 += at(r3, d);
        }
        for (; i < e; ++i) a0 += at(order[i], d);
        sums[(int64_t)c * dim + d] = (a0 + a1) + (a2 + a3);
    }
}

// rows of x packed (row stride dim)
template <typename T>
__device__ __forceinline__ void class_sum_columns(const T* __restrict__ x, int64_t n, int dim, const int* __restrict__ order,
                                                  int c, int64_t b, int64_t e, double* __restrict__ sums) {
    class_sum_columns(x, n, dim, (int64_t)dim, order, c, b, e, sums);
}

// ---------------------------------------------------------------- host side

// class_start [n_classes + 1] on the host: it must run from 0 to n ...
inline int class_start_spans(const int64_t* cs, int n_classes, int64_t n, ErrorChannel& err) {
    if (cs[0] == 0 && cs[n_classes] == n) return XVEC_OK;
    return err.fail(XVEC_ERR_ARG, "class_start must run from 0 to n = %lld (got %lld .. %lld)", (long long)n, (long long)cs[0],
                    (long long)cs[n_classes]);
}

// ... and give every class at least min_rows rows (0: it only must not decrease): the first class that has fewer, or -1.
// The message is the caller's.
inline int first_short_class(const int64_t* cs, int n_classes, int64_t min_rows) {
    for (int c = 0; c < n_classes; ++c)
        if (cs[c + 1] - cs[c] < min_rows) return c;
    return -1;
}

inline int upload_class_start(int64_t* dev, const int64_t* host, int n_classes, hipStream_t s, ErrorChannel& err) {
    return upload(dev, host, (size_t)(n_classes + 1), "class_start", s, err);
}
