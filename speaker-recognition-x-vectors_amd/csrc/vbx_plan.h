// The host side of VBx (csrc/vbx.hip, include/xvec_vbx.h): the argument checks (one text per refusal), the layout of the
// workspace and the launch plan.  Host-compilable (no HIP header, like diar_plan.h), so that tests/test_vbx.py can ask it on
// the CPU (tests/abi/vbx_plan_dump.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/xvec_vbx.h"
#include "rec_plan.h"

namespace xvec {
namespace vbx_plan {

// Columns of a row of rho in the workspace: the dim columns of X * sqrt(phi) and a column of ones behind them, so that the
// product gamma^T rho carries N_s = sum_t gamma_ts in its last column.
inline int64_t rho_cols(int32_t dim) { return (int64_t)dim + 1; }

// rec_start [n_rec + 1]: from 0, every recording with 1 .. XVEC_VBX_MAX_FRAMES frames, fewer than 2^31 in all.
// 0, or 1 with the reason in why.
inline int check_rec_start(const int64_t* rs, int32_t n_rec, Refusal& why) {
    return rec_plan::check_rec_start(rs, n_rec, {"frame", XVEC_VBX_MAX_FRAMES, "XVEC_VBX_MAX_FRAMES"}, why);
}

inline int check_shape(int32_t dim, int32_t n_spk, Refusal& why) {
    if (n_spk < 1 || n_spk > XVEC_VBX_MAX_SPEAKERS)
        return why.refuse("n_spk = %d must lie in 1 .. XVEC_VBX_MAX_SPEAKERS = %d", n_spk, XVEC_VBX_MAX_SPEAKERS);
    if (dim < 1 || dim > XVEC_VBX_MAX_DIM) return why.refuse("dim = %d must lie in 1 .. XVEC_VBX_MAX_DIM = %d", dim, XVEC_VBX_MAX_DIM);
    return 0;
}

inline int check_options(const xvec_vbx_options* o, Refusal& why) {
    if (!o) return why.refuse("null pointer: options");
    if (!(o->loop_prob >= 0.0 && o->loop_prob < 1.0)) return why.refuse("loop_prob = %g must lie in [0, 1)", o->loop_prob);
    if (!(o->Fa > 0.0) || o->Fa * 0.0 != 0.0) return why.refuse("Fa = %g must be positive and finite", o->Fa);
    if (!(o->Fb > 0.0) || o->Fb * 0.0 != 0.0) return why.refuse("Fb = %g must be positive and finite", o->Fb);
    if (o->max_iter < 1) return why.refuse("max_iter = %d: need at least one iteration", o->max_iter);
    if (o->epsilon != o->epsilon) return why.refuse("epsilon is NaN (-inf never stops early)");
    return 0;
}

// Byte offsets of the workspace's parts (each 256-byte aligned) for checked arguments.  Every per-frame part is one array
// over the N frames of the batch: recording r owns the rows rec_start[r] .. rec_start[r + 1] - 1 of it, so a block finds
// its share from rec_start alone.
struct Layout {
    size_t rec_start;      // int64 [n_rec + 1]: the copy of rec_start_host
    size_t rho;            // double [N, dim + 1]: X * sqrt(phi), and a column of ones
    size_t g;              // double [N]: G_t
    size_t em;             // double [N, n_spk]: logp, then the scaled emissions b
    size_t fw;             // double [N, n_spk]: the forward variables a
    size_t c;              // double [N]: the scales c_t
    size_t mx;             // double [N]: the row maxima of logp
    size_t raw;            // int32 [N]: argmax_s gamma_ts before the renumbering
    size_t model;          // double [n_rec, n_spk, dim + 1]: gamma^T rho, then alpha (the last column stays N_s)
    size_t total;
};

inline Layout make_layout(const int64_t* rs, int32_t n_rec, int32_t dim, int32_t n_spk) {
    Layout l{};
    const size_t N = (size_t)rs[n_rec], dp = (size_t)rho_cols(dim), S = (size_t)n_spk;
    Carver c;
    l.rec_start = c.take_bytes(((size_t)n_rec + 1) * sizeof(int64_t));
    l.rho = c.take_bytes(N * dp * sizeof(double));
    l.g = c.take_bytes(N * sizeof(double));
    l.em = c.take_bytes(N * S * sizeof(double));
    l.fw = c.take_bytes(N * S * sizeof(double));
    l.c = c.take_bytes(N * sizeof(double));
    l.mx = c.take_bytes(N * sizeof(double));
    l.raw = c.take_bytes(N * sizeof(int32_t));
    l.model = c.take_bytes((size_t)n_rec * S * dp * sizeof(double));
    l.total = c.total();
    return l;
}

// The launch of xvec_vbx_run: one block per recording, whatever max_iter is; of xvec_vbx_init: a thread per row of gamma and
// per row of pi.
using rec_plan::Launch;

inline Launch run_launch(int32_t n_rec) { return Launch{n_rec, XVEC_VBX_THREADS}; }

inline Launch init_launch(int64_t n_frames, int32_t n_rec) {
    const int64_t rows = n_frames > n_rec ? n_frames : n_rec;
    return Launch{(rows + XVEC_VBX_THREADS - 1) / XVEC_VBX_THREADS, XVEC_VBX_THREADS};
}

}  // namespace vbx_plan
}  // namespace xvec
