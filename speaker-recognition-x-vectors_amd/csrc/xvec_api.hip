// C-ABI layer of libxvec_hip.so (see include/xvec_hip.h): handle, parameter packing,
// workspace planning and the launch sequence of the extraction path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "../../include/xvec_hip.h"
#include "host_support.h"
#include "pool_segments.h"
#include "tdnn_common.h"   // wino_pair_count
#include "xvec_internal.h"

using namespace xvec;

namespace {

thread_local ErrorChannel g_err;

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return g_err.fail(XVEC_ERR_HIP, "%s failed: %s (%s:%d)", #expr,                   \
                              hipGetErrorString(e_), __FILE__, __LINE__);                     \
    } while (0)

// reference main.py:38-44
const int kCtxLen[XVEC_NUM_TDNN] = {5, 3, 3, 1, 1};
const int kCtxDil[XVEC_NUM_TDNN] = {1, 2, 3, 0, 0};

enum { T_L1 = 0, T_POOL = 5, T_SEG6 = 6, T_SEG7 = 7, T_OUT = 8, T_PACK = 9, T_COUNT = 10 };
constexpr int kMaxUtts = 65535;   // utterances per call (16-bit utterance counters in the kernels' row maps)
// fp32 1-tap layers take the bf16_split3 form from this many output rows per CU on (B >= 58 at T = 300).  The form measured
// faster at every batch size down to B = 1; the threshold keeps small batches on the direct form they were
// validated with.
constexpr int kSplit3MinRowsPerCu = 64;
// fp32 3-tap layers take the Winograd form on bf16_split3 operands (tdnn_wino_s3.hip) from this many output rows per CU on, and
// the fp32 Winograd kernel below it (profiles/wino_s3_crossover.txt)
constexpr int kWinoS3MinRowsPerCu = 64;

// The dispatch knobs, read from the environment once, when a handle is created (A/B runs and crossover sweeps, profiles/)
struct Policy {
    int blocks_per_cu;      // XVEC_BLOCKS_PER_CU: persistent TDNN blocks per CU for every kernel, capped at what the kernel holds
                            // (blocks_per_cu below); 0 = unset: each kernel's own (bf16_split3 three, the rest two)
    bool pp;                // XVEC_PP=0 disables the large-batch bf16 mapping (tdnn_pp16.hip) and the streaming layer 1
    int pp_min_tenths;      // XVEC_PP_MIN_TENTHS: ... taken from this many tenths of a 64-frame unit per CU on (18)
    int pp_cu_pct;          // XVEC_PP_CU_PCT (diagnostic): percentage of the CUs the large-batch kernel's grid covers (0 = all)
    bool wino;              // XVEC_WINOGRAD=0 forces the direct form of the fp32 3-tap layers
    bool split3;            // XVEC_SPLIT3=0 forces the direct form of the fp32 1-tap layers
    int split3_min_rows;    // XVEC_SPLIT3_MIN_ROWS: ... which take bf16_split3 from this many output rows per CU on
    bool wino_split3;       // XVEC_WINO_SPLIT3=0 forces the fp32 operands of the Winograd form (tdnn_wino.hip)
    int wino_s3_min_rows;   // XVEC_WINO_SPLIT3_MIN_ROWS: ... which takes bf16_split3 operands from this many output rows per CU on
    // (the next two: tdnn_split3w_knobs, tdnn_split3w.hip)
    bool split3_wide;       // XVEC_SPLIT3_WIDE=0 keeps the pooling bf16_split3 layer on the four-wave kernel (the A/B switch)
    int split3w_min_rows;   // XVEC_SPLIT3_WIDE_MIN_ROWS: ... which takes the 384-channel tile from this many output rows per CU on
                            // (a knob of its own: XVEC_SPLIT3_MIN_ROWS does not move it)
};

int env_int(const char* name, int unset) {
    const char* e = getenv(name);
    return e ? atoi(e) : unset;
}

Policy read_policy() {
    const int tenths = env_int("XVEC_PP_MIN_TENTHS", 18), s3_rows = env_int("XVEC_SPLIT3_MIN_ROWS", kSplit3MinRowsPerCu);
    const int ws3_rows = env_int("XVEC_WINO_SPLIT3_MIN_ROWS", kWinoS3MinRowsPerCu);
    bool s3w_on = true;       // the 384-channel tile's two knobs and its default threshold live with the kernel (tdnn_split3w.hip)
    int s3w_rows = 0;
    tdnn_split3w_knobs(&s3w_on, &s3w_rows);
    return {std::max(0, env_int("XVEC_BLOCKS_PER_CU", 0)), env_int("XVEC_PP", 1) != 0, tenths > 0 ? tenths : 18,
            env_int("XVEC_PP_CU_PCT", 0), env_int("XVEC_WINOGRAD", 1) != 0, env_int("XVEC_SPLIT3", 1) != 0,
            s3_rows >= 0 ? s3_rows : kSplit3MinRowsPerCu, env_int("XVEC_WINO_SPLIT3", 1) != 0,
            ws3_rows >= 0 ? ws3_rows : kWinoS3MinRowsPerCu, s3w_on, s3w_rows};
}

// RAII: the calling thread's current device is whatever it was before the call
struct DeviceGuard {
    int prev = -1;
    bool changed = false;
    hipError_t enter(int dev) {
        hipError_t e = hipGetDevice(&prev);
        if (e != hipSuccess) return e;
        if (prev != dev) {
            e = hipSetDevice(dev);
            changed = e == hipSuccess;
        }
        return e;
    }
    ~DeviceGuard() {
        if (changed) (void)hipSetDevice(prev);
    }
};

}  // namespace

struct xvec_handle {
    xvec_cfg cfg;
    int cin_pad;                       // input_size rounded up to 4 (row stride of layer-1 input)
    TdnnGeom geo[XVEC_NUM_TDNN];
    TdnnGeom geo16[XVEC_NUM_TDNN];     // bf16 packing of layers 2-5: 64-element chunks (layer 1 stays fp32)
    void* Wp16[XVEC_NUM_TDNN];         // bf16, fragment-major
    void* Wp16b;                       // layer 1 only: the same with the bias in the two spare k slots (tdnn_first.hip)
    void* Wr16[XVEC_NUM_TDNN];         // bf16, K-tile major [n_pad/256][k_pad/64][256][64] (tdnn_pp16.hip: both operands reach LDS by DMA)
    void* Wp48[XVEC_NUM_TDNN];         // bf16x3: per chunk W_hi then W_lo fragments (2x the size), fragment-major
    void* Wr48[XVEC_NUM_TDNN];         // bf16x3, K-tile major for tdnn_pp16.hip: per K-tile W_hi | W_lo | W_hi (3x the size of Wr16)
    float* Wp[XVEC_NUM_TDNN];
    float* Wu[XVEC_NUM_TDNN];          // 3-tap layers: Winograd F(2,3) weights U_0..U_3 (tdnn_wino.hip, launch_pack_wino), else null
    void* Wu3[XVEC_NUM_TDNN];          // 3-tap layers: the same U_k as bf16_split3 planes, fragment-major (launch_pack_wino_split3), else null
    void* Wp3[XVEC_NUM_TDNN];          // fp32 1-tap layers 2..5: bf16_split3 weight planes hi | mid | lo, fragment-major (pack.hip), else null
    float* vec[XVEC_NUM_TDNN];         // bias | scale | shift, n_pad each
    // Plain bf16 DEFERS every layer's BatchNorm into its consumer (refold below): layer l stores relu(z + bias'), layer l+1's
    // bf16 weights carry scale_l and its bias' the shift_l (layer 5's BatchNorm goes to pool_finalize as in every mode).
    float* Wraw[XVEC_NUM_TDNN];        // the caller's fp32 weight [cout][taps*cin] and bias, kept for re-folding when the
    float* braw[XVEC_NUM_TDNN];        // producing layer's BatchNorm is (re)loaded later
    float* vec16[XVEC_NUM_TDNN];       // bias' | 1 | 0 (n_pad each): epilogue constants of the plain-bf16 kernels
    bool folded[XVEC_NUM_TDNN];        // Wp16 / Wr16 / vec16 of the layer are consistent with the producing layer's BatchNorm
    hipEvent_t load_evt[XVEC_NUM_TDNN]; // recorded behind a layer's load on the stream that carried it: a re-fold on ANOTHER stream waits for it
    bool tdnn_loaded[XVEC_NUM_TDNN];
    float* affW[3];
    float* affB[3];
    void* affW3[3];                    // affW as bf16 (hi, lo) pairs for the bf16 modes' segment layers (launch_split_pairs); K % 4 == 0
    int affN[3], affK[3];
    bool aff_loaded[3];
    // ragged batches: host offsets staged through pinned memory
    // (allocated once in xvec_create: two slots of kMaxUtts+1 entries, so the ragged entry points
    // never allocate and block only when a third ragged call arrives before the first one's copy left)
    int64_t* offs_pinned[2];
    hipEvent_t offs_evt[2];
    bool offs_pending[2];
    int offs_next;
    int num_cu;
    int split3_blocks_cu;              // blocks of tdnn_split3_kernel the device holds per CU, at most 3 (asked once, xvec_create)
    Policy pol;
    bool wino_s3w_fits;                // the device holds one 512-thread block of tdnn_wino_s3w_kernel per CU (asked once, xvec_create)
    bool split3w_fits;                 // ... and one 768-thread block of tdnn_split3w_kernel
    int last_threads[XVEC_NUM_TDNN], last_blocks[XVEC_NUM_TDNN];   // block size and grid of that launch, where the planner sizes the grid (xvec_get_tdnn_launch)
    int last_kernel[XVEC_NUM_TDNN];    // XVEC_KERNEL_* the last launch of each frame-level layer went to (xvec_get_dispatch)
    int last_form[XVEC_NUM_TDNN];      // XVEC_FORM_* of that launch (xvec_get_tdnn_form)
    int last_operands[XVEC_NUM_TDNN];  // XVEC_OPERANDS_* of that launch (xvec_get_tdnn_operands)
    int last_aff_form[3];              // XVEC_AFFINE_* the last launch of segment_layer6 / 7 / output took, and its K ranges
    int last_aff_ranges[3];            // (xvec_get_affine_dispatch)
    // profiling
    bool profiling;
    hipEvent_t ev0[T_COUNT], ev1[T_COUNT];
    bool ev_used[T_COUNT];
};

namespace {

struct Plan {
    int64_t total, m_pad, rows_alloc;
    size_t xpad, x16, actA, actB, act5, part, part_cnt, pooled, seg6, seg7, offs, bytes;
    int64_t part_slots;
};


Plan make_plan(const xvec_handle* h, int64_t total, int B) {
    Plan p;
    p.total = total;
    p.m_pad = round_up64(total > 0 ? total : 1, 128);
    p.rows_alloc = p.m_pad + kRowPadTail;
    const int nh = h->geo[0].n_pad, n5 = h->geo[4].n_pad;
    size_t o = 0;
    p.xpad = o;   o += align256((size_t)p.rows_alloc * h->cin_pad * 4);
    p.x16 = o;    o += align256((size_t)p.rows_alloc * h->cin_pad * 2 * 2);   // bf16 rows; bf16x3: hi and lo planes
    p.actA = o;   o += align256((size_t)p.rows_alloc * nh * 4);
    p.actB = o;   o += align256((size_t)p.rows_alloc * nh * 4);
    p.act5 = o;   o += align256((size_t)p.rows_alloc * (n5 > nh ? n5 : nh) * 4);   // also the fp32 output of xvec_tdnn_layer
    // pooling partials: one per (32-row group, utterance) -- or, tdnn_pp16.hip, two per (block of a column, utterance)
    p.part_slots = std::max<int64_t>(p.m_pad / 32 + B + 1, 2 * ((int64_t)h->num_cu + B) + 2);
    p.part = o;   o += align256((size_t)p.part_slots * 3 * n5 * 4);   // (addressed with 32-bit offsets: plan_layer checks < 2 GiB)
    p.part_cnt = o; o += align256((size_t)2 * (h->num_cu + B + 2) * 4);     // tdnn_pp16.hip: frames behind each segment partial
    p.pooled = o; o += align256((size_t)B * 2 * XVEC_POOL_CHANNELS * 4);
    p.seg6 = o;   o += align256((size_t)B * h->cfg.x_vector_size * 4);
    p.seg7 = o;   o += align256((size_t)B * h->cfg.x_vector_size * 4);
    p.offs = o;   o += align256((size_t)(B + 1) * 8);
    p.bytes = o;
    return p;
}

// chunk_pair = K elements of two 128-byte chunks (64 for fp32, 128 for bf16): the kernel's main
// loop consumes whole chunk pairs per tap
void fill_geometry(xvec_handle* h, TdnnGeom* geo, int chunk_pair) {
    const int hid = h->cfg.hidden_size;
    for (int i = 0; i < XVEC_NUM_TDNN; ++i) {
        TdnnGeom& g = geo[i];
        g.src_taps = kCtxLen[i];
        g.src_cin = (i == 0) ? h->cfg.input_size : hid;
        g.cin = g.src_cin;
        g.cout = (i == 4) ? XVEC_POOL_CHANNELS : hid;
        g.n_pad = round_up(g.cout, 128);
        g.ctx_span = (kCtxLen[i] - 1) * kCtxDil[i];
        if (kCtxLen[i] == 1 || kCtxDil[i] == 1) {
            // contiguous context: the taps of one output row are one contiguous run of the
            // input buffer (row stride ldx), so they fold into a single tap of K = taps*ldx
            const int ldx = (i == 0) ? h->cin_pad : hid;
            g.n_taps = 1;
            g.tap_rows = 0;
            g.tap_stride_src = (kCtxLen[i] == 1) ? round_up(g.cin, chunk_pair) : ldx;
            g.kpt = (kCtxLen[i] == 1) ? g.cin : kCtxLen[i] * ldx;
        } else {
            g.n_taps = kCtxLen[i];
            g.tap_rows = kCtxDil[i];
            g.kpt = g.cin;
            g.tap_stride_src = round_up(g.cin, chunk_pair);
        }
        g.chunk_k = chunk_pair / 2;
        g.kpt_pad = round_up(g.kpt, chunk_pair);
        g.k_pad = g.n_taps * g.kpt_pad;
    }
}

// The handle's weight buffers on the device and their sizes (0: none), the one list xvec_create allocates and xvec_destroy frees
template <class F>
void each_weight_buffer(xvec_handle* h, F&& f) {
    for (int i = 0; i < XVEC_NUM_TDNN; ++i) {
        const TdnnGeom& g = h->geo[i];
        const size_t w16 = (size_t)h->geo16[i].n_pad * h->geo16[i].k_pad * 2;      // one bf16 copy of the weights
        f(&h->Wp16[i], w16);
        f(&h->Wr16[i], w16);
        f(&h->Wp48[i], 2 * w16);
        f(&h->Wr48[i], 3 * w16);
        f(&h->Wp[i], (size_t)g.n_pad * g.k_pad * 4);
        f(&h->Wu[i], g.n_taps == 3 ? (size_t)g.n_pad * 4 * g.kpt_pad * 4 : 0);
        f(&h->Wu3[i], g.n_taps == 3 ? (size_t)g.n_pad * 4 * g.kpt_pad * 2 * 3 : 0);
        f(&h->Wp3[i], i > 0 && g.n_taps == 1 ? (size_t)g.n_pad * g.k_pad * 2 * 3 : 0);
        f(&h->Wraw[i], (size_t)g.cout * g.src_taps * g.src_cin * 4);
        f(&h->braw[i], (size_t)g.cout * 4);
        f(&h->vec16[i], (size_t)3 * g.n_pad * 4);
        f(&h->vec[i], (size_t)3 * g.n_pad * 4);
    }
    f(&h->Wp16b, (size_t)h->geo16[0].n_pad * h->geo16[0].k_pad * 2);   // layer 1's copy for the streaming kernel (refold)
    for (int i = 0; i < 3; ++i) {
        f(&h->affW[i], (size_t)h->affN[i] * h->affK[i] * 4);
        f(&h->affB[i], (size_t)h->affN[i] * 4);
        f(&h->affW3[i], h->affK[i] % 4 == 0 ? (size_t)h->affN[i] * h->affK[i] * 4 : 0);   // (launch_split_pairs: K % 4 == 0)
    }
}

int aff_index(int which) { return which == XVEC_SEG6 ? 0 : which == XVEC_SEG7 ? 1 : which == XVEC_OUTPUT ? 2 : -1; }

struct StageTimer {
    xvec_handle* h;
    int idx;
    hipStream_t s;
    StageTimer(xvec_handle* h_, int idx_, hipStream_t s_) : h(h_), idx(idx_), s(s_) {
        if (h->profiling) (void)hipEventRecord(h->ev0[idx], s);
    }
    ~StageTimer() {
        if (h->profiling) {
            (void)hipEventRecord(h->ev1[idx], s);
            h->ev_used[idx] = true;
        }
    }
};

// The large-batch mapping (tdnn_pp16.hip) takes a layer when its column count is a multiple of 256 and every CU gets at least
// pp_min_tenths / 10 units of 64 frames (1.8: the crossover with the 128x128 kernel measured in round 3 -- 51 utterances of
// 300 frames for layers 2-4, 18 for layer 5; the same for bf16x3).  Returns the blocks per 256-channel column, 0 if not.
int pp_blocks_per_col(const xvec_handle* h, int n_pad, int64_t rows_out) {
    const Policy& pol = h->pol;
    if (!pol.pp || n_pad % 256 != 0) return 0;
    int bpc = h->num_cu / (n_pad / 256);
    if (pol.pp_cu_pct > 0 && pol.pp_cu_pct < 100) bpc = (bpc * pol.pp_cu_pct + 50) / 100;   // diagnostic knob: fewer, longer row ranges
    const int64_t units = (rows_out + 63) / 64;
    return (bpc >= 1 && units >= bpc && 10 * units >= pol.pp_min_tenths * (int64_t)bpc) ? bpc : 0;
}

// Blocks per CU of a persistent kernel of the 128x128 family: what the kernel holds (bf16_split3: three if the device said so
// when the handle was created, the rest two), or XVEC_BLOCKS_PER_CU capped at that
int blocks_per_cu(const xvec_handle* h, bool split3) {
    const int holds = split3 ? h->split3_blocks_cu : 2;
    return h->pol.blocks_per_cu > 0 ? std::min(h->pol.blocks_per_cu, holds) : holds;
}

// Persistent grid of the 128x128 family (direct, bf16_split3, Winograd) at `per_cu` blocks per CU: blocks per 128-channel
// column, and the period of the CU-pair-aware range sizes, which need the full 2-blocks-per-CU grid and whole XCD runs per
// half (0: off, and always at three blocks per CU).  The kernels split groups_total over these blocks with group_range
// (tdnn_common.h).
void persistent_grid(const xvec_handle* h, int per_cu, int n_tiles, int64_t groups_total, int* blocks_per_col, int* pair_period) {
    const int per_col = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)h->num_cu * per_cu / n_tiles, groups_total));
    const int nwg = per_col * n_tiles;
    const bool ok = per_cu == 2 && nwg == 2 * h->num_cu && nwg % 16 == 0 && (nwg / 8) % (2 * n_tiles) == 0;
    *blocks_per_col = per_col;
    *pair_period = ok ? (nwg / 8) / n_tiles : 0;
}

// One frame-level layer call: what it computes (TdnnMode) and on what.
struct LayerCall {
    int layer;
    TdnnMode mode;
    const void* X;            // input rows (Src::kRows32: the caller's fp32 rows), ldx elements apart
    int ldx;
    int64_t x_rows;           // rows of X that layer 1's guarded reads may reach (0: unguarded)
    void* X16;                // bf16x3 from fp32 rows no kernel of the call reads directly: where their hi / lo split goes
    int64_t x_plane, y_plane; // bf16x3: bytes from the hi to the lo plane of X (of X16 for fp32 rows) / of the output
    void* Y;                  // output rows (Dst::kAct, kF32)
    float* part;              // Dst::kPool: the pooling partials, and the frames behind each (tdnn_pp16.hip)
    int* part_cnt;
    RowMap map;               // row layout of the output
    int64_t rows_out;
};

enum class Launch { kDirect, kPp16, kFirst, kFirst3, kSplit3, kSplit3W, kWino, kWinoS3, kWinoS3W };

// What plan_layer chose for a call: the kernel, its complete arguments, and what the launch reports.
struct LayerPlan {
    int layer;
    Launch launch;
    int kernel, form;         // XVEC_KERNEL_* / XVEC_FORM_* (xvec_get_dispatch / xvec_get_tdnn_form)
    int operands;             // XVEC_OPERANDS_* (xvec_get_tdnn_operands)
    TdnnMode mode;            // the call's; Src::kRows16 when bf16x3 layer 1 reads the split of its rows (the caller makes it)
    TdnnArgs a;
    int64_t pool_units;       // tdnn_pp16.hip pooling: the geometry of its segment partials (finalize_pool)
    int pool_bpc;
};

// The one dispatch decision of the frame-level layers (host code, no HIP calls): the kernel and form of a call, in the order
// pp16 -> first3 / first -> bf16_split3 -> Winograd -> direct (the 128x128 kernel), its complete arguments, and the size limits.
int plan_layer(const xvec_handle* h, const LayerCall& c, LayerPlan& lp) {
    const int l = c.layer;
    const bool bf = c.mode.prec != Prec::kF32, x3 = c.mode.prec == Prec::kBf16x3, pool = c.mode.dst == Dst::kPool;
    const bool from_act = c.mode.src == Src::kAct;
    const TdnnGeom& g = bf ? h->geo16[l] : h->geo[l];
    memset(&lp, 0, sizeof(lp));
    lp.layer = l;
    lp.mode = c.mode;
    lp.kernel = XVEC_KERNEL_TILE128;
    lp.form = XVEC_FORM_DIRECT;
    lp.operands = !bf ? XVEC_OPERANDS_FP32 : x3 ? XVEC_OPERANDS_BF16X3 : XVEC_OPERANDS_BF16;
    TdnnArgs& a = lp.a;
    a.X = c.X;
    a.W = h->Wp[l];
    a.Wf = x3 ? h->Wp48[l] : h->Wp16[l];
    // plain bf16: the folded constants (bias', 1, 0) -- BatchNorm is deferred into the consumer's weights (refold)
    const float* vecs = (bf && !x3) ? h->vec16[l] : h->vec[l];
    a.bias = vecs;
    a.scale = vecs + g.n_pad;
    a.shift = vecs + 2 * g.n_pad;
    a.Y = c.Y;
    a.x_rows = c.x_rows;
    a.ldx = c.ldx;
    a.ldy = g.n_pad;
    a.n_taps = g.n_taps;
    a.tap_rows = g.tap_rows;
    a.kpt = g.kpt;
    a.cpt = g.kpt_pad / (bf ? 2 * kBK : kBK);
    a.k_pad = x3 ? 2 * g.k_pad : g.k_pad;
    a.n_tiles = g.n_pad / 128;
    a.groups_total = (c.rows_out + 31) / 32;
    persistent_grid(h, blocks_per_cu(h, false), a.n_tiles, a.groups_total, &a.blocks_per_col, &a.pair_period);
    a.pool_part = c.part;
    a.pool_cnt = c.part_cnt;
    a.out_map = c.map;
    a.span = h->geo[l].ctx_span;
    a.terms = x3 ? 2 : 1;
    a.y_plane_bytes = x3 ? (int)c.y_plane : 0;
    int bpc = 0;
    if (bf && l > 0 && from_act && c.mode.dst != Dst::kF32 && (bpc = pp_blocks_per_col(h, g.n_pad, c.rows_out))) {
        // bf16, wide layers, enough rows to give every CU about two 64-frame units: the 256-channel ping-pong mapping
        // (tdnn_pp16.hip; bf16x3: the same kernel over three K-tiles per 64-channel slab)
        lp.launch = Launch::kPp16;
        lp.kernel = XVEC_KERNEL_PP;
        a.W = x3 ? h->Wr48[l] : h->Wr16[l];
        a.n_tiles = g.n_pad / 256;
        a.blocks_per_col = lp.pool_bpc = bpc;
        a.groups_total = lp.pool_units = (c.rows_out + 63) / 64;
        a.pair_period = 0;
    } else if (bf && l == 0 && !from_act && c.mode.dst == Dst::kAct && h->pol.pp &&
               (x3 ? tdnn_first3_applicable(a) : tdnn_first_applicable(a))) {
        // layer 1 of the bf16 paths as the streaming kernel (tdnn_first.hip), straight from the fp32 rows
        lp.launch = x3 ? Launch::kFirst3 : Launch::kFirst;
        lp.kernel = XVEC_KERNEL_FIRST;
        if (!x3) a.Wf = h->Wp16b;
    } else if (x3 && c.mode.src == Src::kRows32) {
        // no other kernel reads bf16x3 layer 1 from fp32 rows: the 128x128 kernel reads their hi / lo split
        if (!c.X16) return g_err.fail(XVEC_ERR_STATE, "internal: bf16x3 layer 1 from fp32 rows needs the streaming kernel's shapes");
        lp.mode.src = Src::kRows16;
        a.X = c.X16;
    } else if (!bf && from_act && h->pol.split3 && h->Wp3[l] && c.rows_out >= (int64_t)h->pol.split3_min_rows * h->num_cu) {
        // fp32, one tap (Wp3), large batch: bf16_split3 (tdnn_split3.hip), x = hi + mid + lo and W likewise as bf16 planes, six
        // bf16 products per k-step on the bf16 matrix pipe at 0.375 of the fp32 MFMA time; the same kernel family and epilogues
        lp.launch = Launch::kSplit3;
        lp.form = XVEC_FORM_BF16_SPLIT3;
        lp.operands = XVEC_OPERANDS_BF16_SPLIT3;
        a.terms = 3;
        a.Wf = h->Wp3[l];
        // three blocks per CU (50 688 B of LDS, 168 registers): a third instruction stream per SIMD for the matrix pipe
        persistent_grid(h, blocks_per_cu(h, true), a.n_tiles, a.groups_total, &a.blocks_per_col, &a.pair_period);
        // ... the pooling layer on tiles of 384 channels, twelve waves, one block per CU (tdnn_split3w.hip: a third of the staging
        // work per MFMA; CUs / 4 blocks per column = 3 CUs / 12, the same row ranges, so the same bits) where the width allows,
        // the device holds the block and the batch is large; XVEC_BLOCKS_PER_CU keeps the four-wave grid.  Layer 4 (N = 512)
        // stays on the four-wave kernel.
        if (pool && h->split3w_fits && h->pol.split3_wide && h->pol.blocks_per_cu == 0 && tdnn_split3w_applicable(g) &&
            c.rows_out >= (int64_t)h->pol.split3w_min_rows * h->num_cu) {
            lp.launch = Launch::kSplit3W;
            a.n_tiles = g.n_pad / 384;
            persistent_grid(h, 1, a.n_tiles, a.groups_total, &a.blocks_per_col, &a.pair_period);
        }
    } else if (!bf && from_act && !pool && h->pol.wino && h->Wu[l] && tdnn_wino_applicable(g, c.ldx)) {
        // fp32, three equally spaced taps: Winograd F(2,3) along time (tdnn_wino.hip), 2/3 of the direct form's products; the
        // same kernel family (persistent fp32, 128 x 128 output tiles)
        lp.launch = Launch::kWino;
        lp.form = XVEC_FORM_WINOGRAD_F23;
        a.W = h->Wu[l];
        a.k_pad = 4 * g.kpt_pad;
        // the pair axis (tdnn_wino.hip) instead of the frame axis: its length, with the holes of a ragged batch
        a.p_fixed = c.map.offsets ? 0 : wino_pair_count(c.map.fixed_T - c.map.cum, g.tap_rows);
        const int64_t pairs = c.map.offsets ? (c.rows_out >> 1) + (int64_t)c.map.n_utts * g.tap_rows     // pair_base(n_utts)
                                            : (int64_t)c.map.n_utts * a.p_fixed;
        a.groups_total = (pairs + 31) / 32;
        persistent_grid(h, blocks_per_cu(h, false), a.n_tiles, a.groups_total, &a.blocks_per_col, &a.pair_period);
        if (h->pol.wino_split3 && h->Wu3[l] && tdnn_wino_s3_applicable(g, c.ldx) &&
            c.rows_out >= (int64_t)h->pol.wino_s3_min_rows * h->num_cu) {
            // large batch: the same pairs and grid with bf16_split3 operands (tdnn_wino_s3.hip), 0.375 of the fp32 MFMA time
            lp.launch = Launch::kWinoS3;
            lp.operands = XVEC_OPERANDS_BF16_SPLIT3;
            a.Wf = h->Wu3[l];
            // ... on tiles of 256 channels, eight waves, one block per CU (tdnn_wino_s3w.hip: half the staging work per MFMA,
            // the same bits) where the width allows and the device holds the block; XVEC_BLOCKS_PER_CU=2 keeps the old grid
            if (h->wino_s3w_fits && h->pol.blocks_per_cu <= 1 && tdnn_wino_s3w_applicable(g, c.ldx)) {
                lp.launch = Launch::kWinoS3W;
                a.n_tiles = g.n_pad / 256;
                persistent_grid(h, 1, a.n_tiles, a.groups_total, &a.blocks_per_col, &a.pair_period);
            }
        }
    }
    const bool rows32 = lp.mode.src == Src::kRows32;
    const int64_t x_plane = x3 && !rows32 ? c.x_plane : 0;
    if (x3) {
        a.x_plane_bytes = (int)x_plane;
        a.x_bytes = c.x_rows > 0 && !rows32 ? x_plane + c.x_rows * (int64_t)c.ldx * 2 : 0;   // (fp32 rows: x_rows * ldx * 4)
    }
    // size limits: the kernels address their input with 32-bit byte offsets from a per-tile descriptor, the largest being
    // (rows of a tile + look-ahead + u*span re-basing) * row bytes (+ the lo plane)
    const int64_t es = (bf && !rows32) ? 2 : 4;   // element size of the rows READ
    if (((int64_t)c.map.n_utts * a.span + kRowPadTail) * c.ldx * es + x_plane > 0x7fffffff)
        return g_err.fail(XVEC_ERR_TOO_LARGE, "layer %d: %d utterances x %d channels exceed 32-bit row offsets; split the batch",
                          l, c.map.n_utts, c.ldx);
    if (x3 && (x_plane > 0x3fffffff || c.y_plane > 0x3fffffff))
        return g_err.fail(XVEC_ERR_TOO_LARGE, "batch too large for bf16x3 (plane offsets must fit 30 bits); split it");
    // pooling partials of the 128x128 kernels: one slot per (32-row group, utterance), addressed with 32-bit offsets
    // (tdnn_pp16.hip's segment partials take a 64-bit base per slot and have no such limit)
    if (pool && lp.launch != Launch::kPp16 &&
        (size_t)((c.rows_out + 31) / 32 + c.map.n_utts + 1) * 3 * g.n_pad * 4 > 0x7fffffffull)
        return g_err.fail(XVEC_ERR_TOO_LARGE, "batch too large: pooling partials exceed 2 GiB; split it");
    return XVEC_OK;
}

// Run a planned layer under its stage timer and record what it ran.
int launch_layer(xvec_handle* h, const LayerPlan& lp, hipStream_t s) {
    StageTimer t(h, T_L1 + lp.layer, s);
    const bool pool = lp.mode.dst == Dst::kPool;
    switch (lp.launch) {
        case Launch::kPp16: HIP_TRY(launch_tdnn_pp16(lp.a, pool, s)); break;
        case Launch::kFirst: HIP_TRY(launch_tdnn_first(lp.a, h->num_cu, s)); break;
        case Launch::kFirst3: HIP_TRY(launch_tdnn_first3(lp.a, h->num_cu, s)); break;
        case Launch::kSplit3: HIP_TRY(launch_tdnn_split3(lp.a, pool, s)); break;
        case Launch::kSplit3W: HIP_TRY(launch_tdnn_split3w(lp.a, s)); break;
        case Launch::kWino: HIP_TRY(launch_tdnn_wino(lp.a, s)); break;
        case Launch::kWinoS3: HIP_TRY(launch_tdnn_wino_s3(lp.a, s)); break;
        case Launch::kWinoS3W: HIP_TRY(launch_tdnn_wino_s3w(lp.a, s)); break;
        case Launch::kDirect: HIP_TRY(launch_tdnn(lp.a, lp.mode, s)); break;
    }
    // (the 128x128 family and its 256-channel Winograd tiling; the streaming and ping-pong kernels keep their own block shapes)
    const bool sized = lp.launch != Launch::kFirst && lp.launch != Launch::kFirst3 && lp.launch != Launch::kPp16;
    h->last_threads[lp.layer] = lp.launch == Launch::kSplit3W ? 768 : lp.launch == Launch::kWinoS3W ? 512 : sized ? 256 : 0;
    h->last_blocks[lp.layer] = sized ? lp.a.blocks_per_col * lp.a.n_tiles : 0;
    h->last_kernel[lp.layer] = lp.kernel;
    h->last_form[lp.layer] = lp.form;
    h->last_operands[lp.layer] = lp.operands;
    return XVEC_OK;
}

// (Re)build the plain-bf16 copies of one layer: weights scaled per input channel by the PRODUCING layer's folded BatchNorm
// scale, bias' = bias + W . shift_prev (reference order Linear -> ReLU -> BatchNorm, tdnn_layer.py:30-39: the BatchNorm of
// layer l is an affine map of layer l+1's input, and the valid convolutions have no padded frames where that would differ).
// Needs the layer itself and its producer loaded; xvec_load_tdnn calls it for the layer it loads and for its consumer.
int refold(xvec_handle* h, int layer, hipStream_t s) {
    if (layer < 0 || layer >= XVEC_NUM_TDNN || !h->tdnn_loaded[layer]) return XVEC_OK;
    if (layer > 0 && !h->tdnn_loaded[layer - 1]) { h->folded[layer] = false; return XVEC_OK; }
    // the raw weights of this layer and the folded BatchNorm of its producer may have been written by loads on other streams
    // (ADVICE r04): wait for their events -- no-ops on the stream that recorded them
    HIP_TRY(hipStreamWaitEvent(s, h->load_evt[layer], 0));
    if (layer > 0) HIP_TRY(hipStreamWaitEvent(s, h->load_evt[layer - 1], 0));
    const TdnnGeom& g = h->geo16[layer];
    const float* sc = layer > 0 ? h->vec[layer - 1] + h->geo[layer - 1].n_pad : nullptr;
    const float* sh = layer > 0 ? h->vec[layer - 1] + 2 * h->geo[layer - 1].n_pad : nullptr;
    HIP_TRY(launch_pack_tdnn_bf16(h->Wraw[layer], sc, g, h->Wp16[layer], s));
    HIP_TRY(launch_pack_tdnn_rows_bf16(h->Wraw[layer], sc, g, h->Wr16[layer], s));
    HIP_TRY(launch_fold_bias(h->Wraw[layer], h->braw[layer], sh, g, h->vec16[layer], s));
    if (layer == 0 && g.kpt + 2 <= g.k_pad) {      // the streaming kernel's copy: bias in the spare k slots
        HIP_TRY(launch_pack_tdnn_bf16(h->Wraw[layer], nullptr, g, h->Wp16b, s));
        HIP_TRY(launch_patch_bias_kslots(h->braw[layer], g, h->Wp16b, s));
    }
    h->folded[layer] = true;
    return XVEC_OK;
}

int check_loaded(const xvec_handle* h, int mode) {
    for (int i = 0; i < XVEC_NUM_TDNN; ++i)
        if (!h->tdnn_loaded[i]) return g_err.fail(XVEC_ERR_STATE, "time_context_layers.%d weights not loaded", i);
    for (int i = 0; i < XVEC_NUM_TDNN; ++i)
        if (!h->folded[i]) return g_err.fail(XVEC_ERR_STATE, "internal: time_context_layers.%d not folded", i);
    if (mode == XVEC_MODE_POOLED) return XVEC_OK;
    if (!h->aff_loaded[0]) return g_err.fail(XVEC_ERR_STATE, "segment_layer6 weights not loaded");
    if ((mode == XVEC_MODE_XVEC7 || mode == XVEC_MODE_LOGITS) && !h->aff_loaded[1])
        return g_err.fail(XVEC_ERR_STATE, "segment_layer7 weights not loaded");
    if (mode == XVEC_MODE_LOGITS && !h->aff_loaded[2]) return g_err.fail(XVEC_ERR_STATE, "output weights not loaded");
    return XVEC_OK;
}

// merge the pooling partials planned layer 5 left (in the form of the kernel that wrote them) into pooled[B, 3000]
int finalize_pool(xvec_handle* h, const LayerPlan& l5, float* pooled, hipStream_t s) {
    PoolFinalizeArgs f;
    memset(&f, 0, sizeof(f));
    f.part = l5.a.pool_part;
    f.out = pooled;
    f.map = l5.a.out_map;
    f.C = XVEC_POOL_CHANNELS;
    f.n_pad = h->geo[4].n_pad;
    f.sub_rows = 32;
    f.scale = h->vec[4] + f.n_pad;              // the pooling epilogues leave sums of r = relu(z + bias)
    f.shift = h->vec[4] + 2 * f.n_pad;
    if (l5.kernel == XVEC_KERNEL_PP) {              // tdnn_pp16.hip: one partial per (block, utterance, half)
        f.cnt = l5.a.pool_cnt;
        f.units_total = l5.pool_units;
        f.blocks_per_col = l5.pool_bpc;
    }
    HIP_TRY(launch_pool_finalize(f, s));
    return XVEC_OK;
}

// The five frame-level layers of a batch, planned before anything is enqueued: a batch a size limit refuses leaves the stream
// and the handle as they were.  x_rows: [total, ldx] packed rows (offs_dev == nullptr: B utterances of fixed_T rows each).
// Layer 1 reads the caller's rows (guarded against the end of the buffer and the K tail; bf16 rounds them on the way in,
// bf16x3 reads them as they are or their hi / lo split); every activation buffer holds fp32, bf16 or two bf16 planes in the
// space of one fp32.  Layer 5 carries the statistics-pooling epilogue: its [frames,1500] output stays on chip.
// l5_rows (xvec_forward_segments): layer 5 writes its rows to the act5 region instead -- fp32 with its BatchNorm applied
// (Dst::kF32) in fp32 and bf16x3, its bf16 ReLU output with the BatchNorm left to the pooling (Dst::kAct) in plain bf16.
int plan_stack(const xvec_handle* h, const float* x_rows, int ldx, const int64_t* offs_dev, int B, int fixed_T, const Plan& p,
               int dtype, char* ws, LayerPlan (&lp)[XVEC_NUM_TDNN], bool l5_rows = false) {
    const Prec prec = dtype == XVEC_F32 ? Prec::kF32 : dtype == XVEC_BF16 ? Prec::kBf16 : Prec::kBf16x3;
    if (prec != Prec::kF32 && p.total > 0x7fffffff) return g_err.fail(XVEC_ERR_TOO_LARGE, "too many frames for one bf16 batch; split it");
    const int nh = h->geo[0].n_pad;
    LayerCall c;
    memset(&c, 0, sizeof(c));
    c.mode = {prec, Src::kRows32, Dst::kAct};
    c.X = x_rows;
    c.ldx = ldx;
    c.x_rows = p.total;
    c.X16 = ws + p.x16;
    c.x_plane = p.rows_alloc * (int64_t)ldx * 2;
    // every layer's output is compact: utterance u keeps len_u - cum frames after `cum` frames of
    // context have been consumed (4, 8, 14, 14, 14 after layers 1..5)
    c.map = {offs_dev, B, fixed_T, 0};
    for (int l = 0; l < XVEC_NUM_TDNN; ++l) {
        c.layer = l;
        c.map.cum += h->geo[l].ctx_span;
        c.rows_out = p.total - (int64_t)B * c.map.cum;
        if (l == XVEC_NUM_TDNN - 1 && l5_rows) {
            c.mode.dst = prec == Prec::kBf16 ? Dst::kAct : Dst::kF32;
            c.Y = ws + p.act5;
            c.y_plane = 0;
        } else if (l == XVEC_NUM_TDNN - 1) {
            c.mode.dst = Dst::kPool;
            c.Y = nullptr;
            c.y_plane = 0;
            c.part = reinterpret_cast<float*>(ws + p.part);
            c.part_cnt = reinterpret_cast<int*>(ws + p.part_cnt);
        } else {
            c.Y = ws + (l & 1 ? p.actB : p.actA);
            c.y_plane = p.rows_alloc * (int64_t)nh * 2;          // bytes of one bf16 plane of an activation buffer
        }
        if (int rc = plan_layer(h, c, lp[l])) return rc;
        c.mode.src = Src::kAct;
        c.X = c.Y;
        c.ldx = nh;
        c.x_rows = 0;
        c.x_plane = c.y_plane;
    }
    return XVEC_OK;
}

static_assert(affine_plan::kNone == XVEC_AFFINE_NONE && affine_plan::kTile16 == XVEC_AFFINE_TILE16 &&
              affine_plan::kTile16Elem == XVEC_AFFINE_TILE16_ELEMENTWISE && affine_plan::kSplitK == XVEC_AFFINE_SPLITK &&
              affine_plan::kSplitKX3 == XVEC_AFFINE_SPLITK_BF16X3 && affine_plan::kDirect == XVEC_AFFINE_DIRECT &&
              affine_plan::kDirectX3 == XVEC_AFFINE_DIRECT_BF16X3, "csrc/affine_plan.h and include/xvec_hip.h number the forms alike");

// Segment layer i (0: segment_layer6, 1: segment_layer7, 2: output) on x[M, in]: the one launch_affine_f32 call of the segment
// layers, whoever asks for them.  scr is scratch the split-K forms may overwrite.
int segment_affine(xvec_handle* h, int i, const float* x, int M, int relu, int dtype, float* y, float* scr, size_t scr_bytes,
                   hipStream_t s) {
    // plain bf16 (parity bar 1e-2): the segment layers' products as bf16x3 (affine.hip); XVEC_BF16X3 promises the fp32
    // bar end to end and keeps the fp32 MFMAs here (x3 segment layers measured 3x the fp32 ones' error: 6e-6)
    const bool w3 = dtype == XVEC_BF16;
    affine_plan::Plan ran;
    HIP_TRY(launch_affine_f32(x, h->affW[i], h->affB[i], y, M, h->affN[i], h->affK[i], relu, s, scr, scr_bytes,
                              w3 ? h->affW3[i] : nullptr, &ran));
    h->last_aff_form[i] = ran.form;
    h->last_aff_ranges[i] = ran.S;
    return XVEC_OK;
}

// The segment layers of `mode` (not XVEC_MODE_POOLED) on pooled[M, 3000]: s6 / s7 hold [M, x_vector_size] each, scr is scratch
// the split-K forms may overwrite.
int segment_layers(xvec_handle* h, const float* pooled, int M, float* s6, float* s7, float* scr, size_t scr_bytes, int mode,
                   int dtype, float* out, hipStream_t s) {
    if (mode == XVEC_MODE_XVEC6) {
        StageTimer t(h, T_SEG6, s);
        return segment_affine(h, 0, pooled, M, 0, dtype, out, scr, scr_bytes, s);
    }
    int rc;
    {
        StageTimer t(h, T_SEG6, s);
        if ((rc = segment_affine(h, 0, pooled, M, 1, dtype, s6, scr, scr_bytes, s))) return rc;
    }
    if (mode == XVEC_MODE_XVEC7) {
        StageTimer t(h, T_SEG7, s);
        return segment_affine(h, 1, s6, M, 0, dtype, out, scr, scr_bytes, s);
    }
    {
        StageTimer t(h, T_SEG7, s);
        if ((rc = segment_affine(h, 1, s6, M, 1, dtype, s7, scr, scr_bytes, s))) return rc;
    }
    {
        StageTimer t(h, T_OUT, s);
        if ((rc = segment_affine(h, 2, s7, M, 0, dtype, out, scr, scr_bytes, s))) return rc;
    }
    return XVEC_OK;
}

// Run the planned stack (x_rows, ldx as planned) and the segment layers of `mode`.
int forward_rows(xvec_handle* h, const LayerPlan (&lp)[XVEC_NUM_TDNN], const float* x_rows, int ldx, int B, const Plan& p,
                 int mode, int dtype, float* out, char* ws, hipStream_t s) {
    float* pooled = mode == XVEC_MODE_POOLED ? out : reinterpret_cast<float*>(ws + p.pooled);
    int rc;
    if (lp[0].mode.src == Src::kRows16) {    // [total, ldx] fp32 -> bf16 hi and lo planes (same row stride in elements)
        StageTimer t(h, T_PACK, s);
        HIP_TRY(launch_pack_rows_split(x_rows, p.total, ldx, ldx, lp[0].a.x_plane_bytes / 2, ws + p.x16, s));
    }
    for (const LayerPlan& l : lp)
        if ((rc = launch_layer(h, l, s))) return rc;
    {
        StageTimer t(h, T_POOL, s);
        if ((rc = finalize_pool(h, lp[XVEC_NUM_TDNN - 1], pooled, s))) return rc;
    }
    if (mode == XVEC_MODE_POOLED) return XVEC_OK;
    // the frame-level activations are dead from here on: layers 1-4's buffers serve as split-K scratch (actA and actB are adjacent)
    return segment_layers(h, pooled, B, reinterpret_cast<float*>(ws + p.seg6), reinterpret_cast<float*>(ws + p.seg7),
                          reinterpret_cast<float*>(ws + p.actA), (p.actB - p.actA) * 2, mode, dtype, out, s);
}

// Workspace of xvec_forward_segments: the plan of the batch, and behind it the segments' rows, pooled statistics and
// segment-layer activations (M = n_segments rows each).
struct SegPlan {
    Plan p;
    size_t seg_row, seg_n, pooled, seg6, seg7, bytes;
};

constexpr int64_t kMaxSegments = 65535 * 16;   // per call: the segment layers' direct form puts ceil(M / 16) on grid.y

SegPlan make_seg_plan(const xvec_handle* h, int64_t total, int B, int64_t n_segments) {
    SegPlan sp;
    sp.p = make_plan(h, total, B);
    size_t o = sp.p.bytes;
    sp.seg_row = o; o += align256((size_t)n_segments * 8);
    sp.seg_n = o;   o += align256((size_t)n_segments * 4);
    sp.pooled = o;  o += align256((size_t)n_segments * 2 * XVEC_POOL_CHANNELS * 4);
    sp.seg6 = o;    o += align256((size_t)n_segments * h->cfg.x_vector_size * 4);
    sp.seg7 = o;    o += align256((size_t)n_segments * h->cfg.x_vector_size * 4);
    sp.bytes = o;
    return sp;
}

// host offsets -> device (stream ordered, via the handle's ring of two pinned staging slots).
// Synchronous part: only when both slots still hold copies that have not left them (a third ragged
// call enqueued before the first one's copy ran) does this wait for the older one.
int stage_offsets(xvec_handle* h, const int64_t* offs_host, const int32_t* lengths_host, int B, int64_t* dev,
                  hipStream_t s) {
    const size_t n = (size_t)B + 1;
    const int slot = h->offs_next;
    h->offs_next ^= 1;
    if (h->offs_pending[slot]) {
        HIP_TRY(hipEventSynchronize(h->offs_evt[slot]));
        h->offs_pending[slot] = false;
    }
    int64_t* pin = h->offs_pinned[slot];        // free: its last copy has left it
    if (offs_host) {
        memcpy(pin, offs_host, n * 8);
    } else {                                    // prefix sum of the lengths, built in place (no host allocation)
        pin[0] = 0;
        for (int i = 0; i < B; ++i) pin[i + 1] = pin[i] + lengths_host[i];
    }
    HIP_TRY(hipMemcpyAsync(dev, pin, n * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(h->offs_evt[slot], s));
    h->offs_pending[slot] = true;
    return XVEC_OK;
}

int common_checks(xvec_handle* h, const void* x, int B, int mode, int dtype, const void* out, const void* ws) {
    if (!h) return g_err.fail(XVEC_ERR_ARG, "null handle");
    if (!x || !out || !ws) return g_err.fail(XVEC_ERR_ARG, "null tensor pointer");
    if (B < 1) return g_err.fail(XVEC_ERR_ARG, "B must be in [1, %d] (got %d)", kMaxUtts, B);
    if (B > kMaxUtts) return g_err.fail(XVEC_ERR_TOO_LARGE, "B must be in [1, %d] (got %d); split larger batches", kMaxUtts, B);
    if (mode != XVEC_MODE_LOGITS && mode != XVEC_MODE_XVEC6 && mode != XVEC_MODE_XVEC7 && mode != XVEC_MODE_POOLED)
        return g_err.fail(XVEC_ERR_ARG, "unknown mode %d", mode);
    if (dtype != XVEC_F32 && dtype != XVEC_BF16 && dtype != XVEC_BF16X3) return g_err.fail(XVEC_ERR_ARG, "unknown dtype %d", dtype);
    if ((reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(ws) & 255))
        return g_err.fail(XVEC_ERR_ARG, "x must be 16-byte and workspace 256-byte aligned");
    return check_loaded(h, mode);
}

// The per-layer entries' common part: arguments, handle state, workspace, and the call on x staged into the layer's native row
// layout (stride = the producer's n_pad; layer 1: fp32 rows padded to cin_pad).  B and T are checked by the caller.
int layer_entry(const xvec_handle* h, int layer, const void* x, const void* out, int B, int T, int dtype, void* workspace,
                size_t workspace_bytes, Plan& p, LayerCall& c) {
    if (!x || !out || !workspace) return g_err.fail(XVEC_ERR_ARG, "null tensor pointer");
    if (dtype != XVEC_F32 && dtype != XVEC_BF16 && dtype != XVEC_BF16X3) return g_err.fail(XVEC_ERR_ARG, "unknown dtype %d", dtype);
    if (!h->tdnn_loaded[layer]) return g_err.fail(XVEC_ERR_STATE, "time_context_layers.%d weights not loaded", layer);
    if (dtype == XVEC_BF16 && !h->folded[layer])
        return g_err.fail(XVEC_ERR_STATE, "time_context_layers.%d: plain bf16 folds the BatchNorm of layer %d into it; load that layer too", layer, layer - 1);
    p = make_plan(h, (int64_t)B * T, B);
    if (workspace_bytes < p.bytes)
        return g_err.fail(XVEC_ERR_WORKSPACE, "workspace too small: %zu < %zu", workspace_bytes, p.bytes);
    char* ws = static_cast<char*>(workspace);
    const bool x3 = dtype == XVEC_BF16X3;
    const int span = h->geo[layer].ctx_span;
    memset(&c, 0, sizeof(c));
    c.layer = layer;
    c.mode = {dtype == XVEC_F32 ? Prec::kF32 : x3 ? Prec::kBf16x3 : Prec::kBf16, layer == 0 ? Src::kRows32 : Src::kAct, Dst::kF32};
    c.ldx = layer == 0 ? h->cin_pad : h->geo[layer - 1].n_pad;
    c.X = ws + (layer > 0 ? p.actA : x3 ? p.actB : p.xpad);    // (bf16x3 layer 1: the fp32 rows its hi / lo split is made from)
    c.x_rows = p.total;
    c.X16 = ws + p.x16;
    c.x_plane = x3 ? p.rows_alloc * (int64_t)c.ldx * 2 : 0;
    c.map = {nullptr, B, T, span};
    c.rows_out = (int64_t)B * (T - span);
    return XVEC_OK;
}

// Stage a per-layer entry's input x[B,T,cin] where its planned layer reads it: bf16 / two bf16 planes as in xvec_forward.
int stage_layer_input(const xvec_handle* h, const LayerCall& c, const LayerPlan& lp, const float* x, int B, int T, const Plan& p,
                      char* ws, hipStream_t s) {
    const int l = c.layer, cin = h->geo[l].src_cin;
    if (c.mode.prec == Prec::kBf16x3) {     // fp32 rows first (padding to ldx), then the hi / lo split unless the layer reads those
        float* x32 = reinterpret_cast<float*>(ws + p.actB);
        HIP_TRY(launch_pack_rows(x, nullptr, B, T, cin, c.ldx, x32, false, s));
        if (lp.mode.src != Src::kRows32)
            HIP_TRY(launch_pack_rows_split(x32, p.total, c.ldx, c.ldx, c.x_plane / 2, const_cast<void*>(lp.a.X), s));
        return XVEC_OK;
    }
    // plain bf16, layers 2-5: the kernel reads the producing layer's relu output and carries that layer's BatchNorm in its
    // weights (refold), so the caller's x -- the reference's layer input, BatchNorm applied -- is taken back through it
    // (layer 1 reads fp32 rows and rounds them itself, exactly as in xvec_forward)
    const bool b16 = c.mode.prec == Prec::kBf16 && l > 0;
    const float* un = b16 ? h->vec[l - 1] : nullptr;
    const int npp = b16 ? h->geo[l - 1].n_pad : 0;
    HIP_TRY(launch_pack_rows(x, nullptr, B, T, cin, c.ldx, const_cast<void*>(c.X), b16, s, un ? un + npp : nullptr,
                             un ? un + 2 * npp : nullptr));
    return XVEC_OK;
}

}  // namespace

extern "C" {

const char* xvec_last_error(void) { return g_err.c_str(); }
#ifndef XVEC_BUILD_ID
#define XVEC_BUILD_ID "unknown"
#endif
const char* xvec_version(void) { return "xvec_hip gfx950 build " XVEC_BUILD_ID; }

int xvec_create(const xvec_cfg* cfg, xvec_handle** out) {
    if (!cfg || !out) return g_err.fail(XVEC_ERR_ARG, "null argument");
    if (cfg->input_size < 1 || cfg->hidden_size < 1 || cfg->num_classes < 1 || cfg->x_vector_size < 1)
        return g_err.fail(XVEC_ERR_ARG, "sizes must be positive");
    if (cfg->hidden_size > 8192 || cfg->input_size > 8192)
        return g_err.fail(XVEC_ERR_ARG, "input_size / hidden_size above 8192 are not supported (32-bit row offsets)");
    DeviceGuard guard;                 // allocate on cfg->device, leave the caller's current device as it was
    HIP_TRY(guard.enter(cfg->device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, cfg->device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return g_err.fail(XVEC_ERR_STATE, "device %d is %s; this library is built for gfx950 only", cfg->device,
                          prop.gcnArchName);
    xvec_handle* h = new (std::nothrow) xvec_handle();
    if (!h) return g_err.fail(XVEC_ERR_STATE, "out of host memory");
    memset(h, 0, sizeof(*h));
    h->cfg = *cfg;
    h->num_cu = device_cu_count();
    h->pol = read_policy();
    // three persistent blocks of the split form per CU only where the device really holds them: 768 blocks on a CU that takes
    // two at a time would run in two rounds
    int s3_blocks = 0;
    if (hipError_t e = tdnn_split3_max_blocks_per_cu(&s3_blocks); e != hipSuccess) {
        delete h;
        return g_err.fail(XVEC_ERR_HIP, "occupancy query of tdnn_split3_kernel failed: %s", hipGetErrorString(e));
    }
    h->split3_blocks_cu = std::max(1, std::min(3, s3_blocks));
    // ... and the eight-wave Winograd split3 block only where one fits
    int s3w_blocks = 0;
    if (hipError_t e = tdnn_wino_s3w_max_blocks_per_cu(&s3w_blocks); e != hipSuccess) {
        delete h;
        return g_err.fail(XVEC_ERR_HIP, "occupancy query of tdnn_wino_s3w_kernel failed: %s", hipGetErrorString(e));
    }
    h->wino_s3w_fits = s3w_blocks >= 1;
    // ... and the twelve-wave split3 pooling block
    int s3wide_blocks = 0;
    if (hipError_t e = tdnn_split3w_max_blocks_per_cu(&s3wide_blocks); e != hipSuccess) {
        delete h;
        return g_err.fail(XVEC_ERR_HIP, "occupancy query of tdnn_split3w_kernel failed: %s", hipGetErrorString(e));
    }
    h->split3w_fits = s3wide_blocks >= 1;
    h->cin_pad = round_up(cfg->input_size, 4);
    fill_geometry(h, h->geo, 2 * kBK);
    fill_geometry(h, h->geo16, 4 * kBK);
    const int N[3] = {cfg->x_vector_size, cfg->x_vector_size, cfg->num_classes};
    const int K[3] = {2 * XVEC_POOL_CHANNELS, cfg->x_vector_size, cfg->x_vector_size};
    std::copy(N, N + 3, h->affN);
    std::copy(K, K + 3, h->affK);
    bool ok = true;
    each_weight_buffer(h, [&](auto** ptr, size_t bytes) {
        ok = ok && (bytes == 0 || hipMalloc(reinterpret_cast<void**>(ptr), bytes) == hipSuccess);
    });
    if (!ok) {
        xvec_destroy(h);
        return g_err.fail(XVEC_ERR_HIP, "hipMalloc of packed weights failed");
    }
    for (int i = 0; i < 2 && ok; ++i)
        ok = hipEventCreateWithFlags(&h->offs_evt[i], hipEventDisableTiming) == hipSuccess &&
             hipHostMalloc(reinterpret_cast<void**>(&h->offs_pinned[i]), (size_t)(kMaxUtts + 1) * 8,
                           hipHostMallocDefault) == hipSuccess;
    for (int i = 0; i < T_COUNT && ok; ++i)
        ok = hipEventCreate(&h->ev0[i]) == hipSuccess && hipEventCreate(&h->ev1[i]) == hipSuccess;
    for (int i = 0; i < XVEC_NUM_TDNN && ok; ++i)
        ok = hipEventCreateWithFlags(&h->load_evt[i], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        xvec_destroy(h);
        return g_err.fail(XVEC_ERR_HIP, "hipEventCreate / hipHostMalloc failed");
    }
    *out = h;
    return XVEC_OK;
}

void xvec_destroy(xvec_handle* h) {
    if (!h) return;
    each_weight_buffer(h, [](auto** ptr, size_t) {
        if (*ptr) (void)hipFree(*ptr);
        *ptr = nullptr;
    });
    for (int i = 0; i < 2; ++i) {
        if (h->offs_pinned[i]) (void)hipHostFree(h->offs_pinned[i]);
        if (h->offs_evt[i]) (void)hipEventDestroy(h->offs_evt[i]);
    }
    for (int i = 0; i < XVEC_NUM_TDNN; ++i)
        if (h->load_evt[i]) (void)hipEventDestroy(h->load_evt[i]);
    for (int i = 0; i < T_COUNT; ++i) {
        if (h->ev0[i]) (void)hipEventDestroy(h->ev0[i]);
        if (h->ev1[i]) (void)hipEventDestroy(h->ev1[i]);
    }
    delete h;
}

int xvec_load_tdnn(xvec_handle* h, int layer, const float* weight, const float* bias, const float* bn_weight,
                   const float* bn_bias, const float* bn_mean, const float* bn_var, float eps, xvec_stream stream) {
    if (!h || layer < 0 || layer >= XVEC_NUM_TDNN) return g_err.fail(XVEC_ERR_ARG, "bad handle or layer %d", layer);
    if (!weight || !bias) return g_err.fail(XVEC_ERR_ARG, "null weight/bias");
    DeviceGuard guard;                 // launches go to the handle's device whatever the caller's current one is
    HIP_TRY(guard.enter(h->cfg.device));
    const bool has_bn = bn_weight && bn_bias && bn_mean && bn_var;
    const bool none_bn = !bn_weight && !bn_bias && !bn_mean && !bn_var;
    if (h->cfg.batch_norm ? !has_bn : !none_bn)
        return g_err.fail(XVEC_ERR_ARG, "BatchNorm tensors must be %s for batch_norm=%d",
                          h->cfg.batch_norm ? "all given" : "all NULL", h->cfg.batch_norm);
    const TdnnGeom& g = h->geo[layer];
    // A RE-load of this layer while a neighbour's load is still in flight on another stream: that load's re-folds read
    // Wraw / vec of this layer (refold(layer) reads the producer's BatchNorm, refold(layer + 1) this layer's), which the writes
    // below replace -- they wait for the neighbours' loads first (a first load has nothing to wait for).
    if (layer > 0 && h->tdnn_loaded[layer - 1]) HIP_TRY(hipStreamWaitEvent(static_cast<hipStream_t>(stream), h->load_evt[layer - 1], 0));
    if (layer + 1 < XVEC_NUM_TDNN && h->tdnn_loaded[layer + 1])
        HIP_TRY(hipStreamWaitEvent(static_cast<hipStream_t>(stream), h->load_evt[layer + 1], 0));
    HIP_TRY(launch_pack_tdnn(weight, bias, bn_weight, bn_bias, bn_mean, bn_var, eps, g, h->Wp[layer],
                             h->vec[layer], h->vec[layer] + g.n_pad, h->vec[layer] + 2 * g.n_pad,
                             static_cast<hipStream_t>(stream)));
    if (h->Wu[layer]) HIP_TRY(launch_pack_wino(weight, g, h->Wu[layer], static_cast<hipStream_t>(stream)));
    if (h->Wu3[layer]) HIP_TRY(launch_pack_wino_split3(weight, g, h->Wu3[layer], static_cast<hipStream_t>(stream)));
    if (h->Wp3[layer]) HIP_TRY(launch_pack_tdnn_split3(weight, g, h->Wp3[layer], static_cast<hipStream_t>(stream)));
    HIP_TRY(launch_pack_tdnn_rows_bf16x3(weight, h->geo16[layer], h->Wr48[layer], static_cast<hipStream_t>(stream)));
    {
        TdnnGeom g3 = h->geo16[layer];
        g3.terms = 2;
        HIP_TRY(launch_pack_tdnn_bf16(weight, nullptr, g3, h->Wp48[layer], static_cast<hipStream_t>(stream)));
    }
    // plain bf16 (BatchNorm deferred into the consumer): this layer's copies depend on its producer's BatchNorm, its
    // consumer's on this layer's -- whatever the order the layers are loaded in
    HIP_TRY(hipMemcpyAsync(h->Wraw[layer], weight, (size_t)g.cout * g.src_taps * g.src_cin * 4, hipMemcpyDeviceToDevice,
                           static_cast<hipStream_t>(stream)));
    HIP_TRY(hipMemcpyAsync(h->braw[layer], bias, (size_t)g.cout * 4, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    h->tdnn_loaded[layer] = true;
    HIP_TRY(hipEventRecord(h->load_evt[layer], static_cast<hipStream_t>(stream)));
    if (int rc = refold(h, layer, static_cast<hipStream_t>(stream))) return rc;
    if (int rc = refold(h, layer + 1, static_cast<hipStream_t>(stream))) return rc;
    // (the re-folds above read what this call wrote: later loads of the neighbours on other streams wait for them too)
    HIP_TRY(hipEventRecord(h->load_evt[layer], static_cast<hipStream_t>(stream)));
    return XVEC_OK;
}

int xvec_load_affine(xvec_handle* h, int which, const float* weight, const float* bias, xvec_stream stream) {
    const int i = aff_index(which);
    if (!h || i < 0) return g_err.fail(XVEC_ERR_ARG, "bad handle or affine id %d", which);
    if (!weight || !bias) return g_err.fail(XVEC_ERR_ARG, "null weight/bias");
    DeviceGuard guard;                 // launches go to the handle's device whatever the caller's current one is
    HIP_TRY(guard.enter(h->cfg.device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemcpyAsync(h->affW[i], weight, (size_t)h->affN[i] * h->affK[i] * 4, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(h->affB[i], bias, (size_t)h->affN[i] * 4, hipMemcpyDeviceToDevice, s));
    if (h->affW3[i]) HIP_TRY(launch_split_pairs(h->affW[i], h->affW3[i], (int64_t)h->affN[i] * h->affK[i], s));
    h->aff_loaded[i] = true;
    return XVEC_OK;
}

size_t xvec_workspace_bytes(const xvec_handle* h, int64_t total_frames, int32_t n_utts) {
    if (!h || total_frames < 1 || n_utts < 1) return 0;
    return make_plan(h, total_frames, n_utts).bytes;
}

int xvec_workspace_layout(const xvec_handle* h, int64_t total_frames, int32_t n_utts, xvec_ws_layout* out) {
    if (!h || !out || total_frames < 1 || n_utts < 1) return g_err.fail(XVEC_ERR_ARG, "bad argument");
    const Plan p = make_plan(h, total_frames, n_utts);
    out->act_a = p.actA;
    out->act_b = p.actB;
    out->part = p.part;
    out->part_cnt = p.part_cnt;
    out->pooled = p.pooled;
    out->bytes = p.bytes;
    out->rows_alloc = p.rows_alloc;
    out->part_slots = p.part_slots;
    out->pool_n_pad = h->geo[4].n_pad;
    out->hidden_n_pad = h->geo[0].n_pad;
    out->num_cu = h->num_cu;
    return XVEC_OK;
}

int xvec_forward(xvec_handle* h, const float* x, const int32_t* lengths_host, int32_t B, int32_t T, int mode,
                 int dtype, float* out, void* workspace, size_t workspace_bytes, xvec_stream stream) {
    int rc = common_checks(h, x, B, mode, dtype, out, workspace);
    if (rc) return rc;
    DeviceGuard guard;                 // launches go to the handle's device whatever the caller's current one is
    HIP_TRY(guard.enter(h->cfg.device));
    if (T <= XVEC_TOTAL_CONTEXT)
        return g_err.fail(XVEC_ERR_ARG, "T=%d: need at least %d frames (receptive field of the TDNN stack)", T,
                          XVEC_TOTAL_CONTEXT + 1);
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    const int C = h->cfg.input_size;

    if (!lengths_host) {
        const Plan p = make_plan(h, (int64_t)B * T, B);
        if (workspace_bytes < p.bytes)
            return g_err.fail(XVEC_ERR_WORKSPACE, "workspace too small: %zu < %zu", workspace_bytes, p.bytes);
        float* xp = reinterpret_cast<float*>(ws + p.xpad);
        const bool pad = h->cin_pad != C;                 // channel count not a multiple of 4: pad rows once
        const float* rows = pad ? xp : x;
        LayerPlan lp[XVEC_NUM_TDNN];
        if ((rc = plan_stack(h, rows, h->cin_pad, nullptr, B, T, p, dtype, ws, lp))) return rc;
        if (pad) {
            StageTimer t(h, T_PACK, s);
            HIP_TRY(launch_pack_rows(x, nullptr, B, T, C, h->cin_pad, xp, false, s));
        }
        return forward_rows(h, lp, rows, h->cin_pad, B, p, mode, dtype, out, ws, s);
    }

    // ragged: pack the valid frames, run the stack on sum(lengths) rows only
    int64_t total = 0;
    for (int i = 0; i < B; ++i) {
        const int n = lengths_host[i];
        if (n <= XVEC_TOTAL_CONTEXT || n > T)
            return g_err.fail(XVEC_ERR_ARG, "lengths[%d]=%d outside [%d, T=%d]", i, n, XVEC_TOTAL_CONTEXT + 1, T);
        total += n;
    }
    const Plan p = make_plan(h, total, B);
    if (workspace_bytes < p.bytes)
        return g_err.fail(XVEC_ERR_WORKSPACE, "workspace too small: %zu < %zu", workspace_bytes, p.bytes);
    int64_t* offs_dev = reinterpret_cast<int64_t*>(ws + p.offs);
    float* xp = reinterpret_cast<float*>(ws + p.xpad);
    LayerPlan lp[XVEC_NUM_TDNN];
    if ((rc = plan_stack(h, xp, h->cin_pad, offs_dev, B, 0, p, dtype, ws, lp))) return rc;
    if ((rc = stage_offsets(h, nullptr, lengths_host, B, offs_dev, s))) return rc;
    {
        StageTimer t(h, T_PACK, s);
        HIP_TRY(launch_pack_rows(x, offs_dev, B, T, C, h->cin_pad, xp, false, s));
    }
    return forward_rows(h, lp, xp, h->cin_pad, B, p, mode, dtype, out, ws, s);
}

int xvec_forward_packed(xvec_handle* h, const float* x_packed, const int64_t* offsets_host, int32_t B, int mode,
                        int dtype, float* out, void* workspace, size_t workspace_bytes, xvec_stream stream) {
    int rc = common_checks(h, x_packed, B, mode, dtype, out, workspace);
    if (rc) return rc;
    DeviceGuard guard;                 // launches go to the handle's device whatever the caller's current one is
    HIP_TRY(guard.enter(h->cfg.device));
    if (!offsets_host) return g_err.fail(XVEC_ERR_ARG, "null offsets");
    if (offsets_host[0] != 0) return g_err.fail(XVEC_ERR_ARG, "offsets[0] must be 0");
    for (int i = 0; i < B; ++i) {
        const int64_t n = offsets_host[i + 1] - offsets_host[i];
        if (n <= XVEC_TOTAL_CONTEXT)
            return g_err.fail(XVEC_ERR_ARG, "utterance %d has %lld frames; need at least %d", i, (long long)n,
                              XVEC_TOTAL_CONTEXT + 1);
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    const int64_t total = offsets_host[B];
    const Plan p = make_plan(h, total, B);
    if (workspace_bytes < p.bytes)
        return g_err.fail(XVEC_ERR_WORKSPACE, "workspace too small: %zu < %zu", workspace_bytes, p.bytes);
    const int C = h->cfg.input_size;
    int64_t* offs_dev = reinterpret_cast<int64_t*>(ws + p.offs);
    float* xp = reinterpret_cast<float*>(ws + p.xpad);
    const bool pad = h->cin_pad != C;
    if (pad && total > 0x7fffffff) return g_err.fail(XVEC_ERR_ARG, "too many frames");
    const float* rows = pad ? xp : x_packed;
    LayerPlan lp[XVEC_NUM_TDNN];
    if ((rc = plan_stack(h, rows, h->cin_pad, offs_dev, B, 0, p, dtype, ws, lp))) return rc;
    if ((rc = stage_offsets(h, offsets_host, nullptr, B, offs_dev, s))) return rc;
    if (pad) {
        StageTimer t(h, T_PACK, s);
        HIP_TRY(launch_pack_rows(x_packed, nullptr, 1, (int)total, C, h->cin_pad, xp, false, s));
    }
    return forward_rows(h, lp, rows, h->cin_pad, B, p, mode, dtype, out, ws, s);
}

size_t xvec_segments_workspace_bytes(const xvec_handle* h, int64_t total_frames, int32_t n_utts, int64_t n_segments) {
    if (!h || total_frames < 1 || n_utts < 1 || n_segments < 1 || n_segments > kMaxSegments) return 0;
    return make_seg_plan(h, total_frames, n_utts, n_segments).bytes;
}

int xvec_stat_pool_segments(const void* y, int elem, int64_t rows, int32_t ldy, int32_t C, const int64_t* seg_row_dev,
                            const int32_t* seg_n_dev, int64_t n_segments, const float* scale_dev, const float* shift_dev,
                            float* out, xvec_stream stream) {
    if (!y || !seg_row_dev || !seg_n_dev || !out) return g_err.fail(XVEC_ERR_ARG, "null tensor pointer");
    if (elem != 0 && elem != 1) return g_err.fail(XVEC_ERR_ARG, "elem must be 0 (fp32) or 1 (bf16), got %d", elem);
    if (rows < 1 || C < 1 || ldy < C) return g_err.fail(XVEC_ERR_ARG, "need rows >= 1 and 1 <= C <= ldy (got rows=%lld C=%d ldy=%d)", (long long)rows, C, ldy);
    if (n_segments < 1 || n_segments > 0x7fffffff) return g_err.fail(XVEC_ERR_ARG, "n_segments must be in [1, 2^31) (got %lld)", (long long)n_segments);
    if (!scale_dev != !shift_dev) return g_err.fail(XVEC_ERR_ARG, "scale and shift go together");
    if (reinterpret_cast<uintptr_t>(y) % (elem ? 2 : 4)) return g_err.fail(XVEC_ERR_ARG, "y is not aligned to its element size");
    PoolSegArgs a;
    memset(&a, 0, sizeof(a));
    a.y = y;
    a.elem = elem;
    a.rows = rows;
    a.ldy = ldy;
    a.C = C;
    a.row0 = seg_row_dev;
    a.n = seg_n_dev;
    a.n_segments = n_segments;
    a.scale = scale_dev;
    a.shift = shift_dev;
    a.out = out;
    HIP_TRY(launch_pool_segments(a, static_cast<hipStream_t>(stream)));
    return XVEC_OK;
}

int xvec_stat_pool_segments_vector(const void* y, int elem, int32_t ldy, int32_t C) {
    if (!y || (elem != 0 && elem != 1) || C < 1 || ldy < C) return -1;
    return pool_segments_vector(y, elem, ldy, C) ? 1 : 0;
}

int xvec_forward_segments(xvec_handle* h, const float* x_packed, const int64_t* offsets_host, int32_t B,
                          const int32_t* seg_utt_dev, const int32_t* seg_start_dev, const int32_t* seg_len_dev,
                          int64_t n_segments, int mode, int dtype, float* out, void* workspace, size_t workspace_bytes,
                          xvec_stream stream) {
    int rc = common_checks(h, x_packed, B, mode, dtype, out, workspace);
    if (rc) return rc;
    if (!offsets_host) return g_err.fail(XVEC_ERR_ARG, "null offsets");
    if (!seg_utt_dev || !seg_start_dev || !seg_len_dev) return g_err.fail(XVEC_ERR_ARG, "null segment array");
    if (n_segments < 1) return g_err.fail(XVEC_ERR_ARG, "n_segments must be at least 1 (got %lld)", (long long)n_segments);
    if (n_segments > kMaxSegments)
        return g_err.fail(XVEC_ERR_TOO_LARGE, "at most %lld segments per call (got %lld); split the list", (long long)kMaxSegments,
                          (long long)n_segments);
    DeviceGuard guard;                 // launches go to the handle's device whatever the caller's current one is
    HIP_TRY(guard.enter(h->cfg.device));
    if (offsets_host[0] != 0) return g_err.fail(XVEC_ERR_ARG, "offsets[0] must be 0");
    for (int i = 0; i < B; ++i) {
        const int64_t n = offsets_host[i + 1] - offsets_host[i];
        if (n <= XVEC_TOTAL_CONTEXT)
            return g_err.fail(XVEC_ERR_ARG, "recording %d has %lld frames; need at least %d", i, (long long)n, XVEC_TOTAL_CONTEXT + 1);
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    const int64_t total = offsets_host[B];
    const SegPlan sp = make_seg_plan(h, total, B, n_segments);
    const Plan& p = sp.p;
    if (workspace_bytes < sp.bytes)
        return g_err.fail(XVEC_ERR_WORKSPACE, "workspace too small: %zu < %zu", workspace_bytes, sp.bytes);
    const int C = h->cfg.input_size;
    int64_t* offs_dev = reinterpret_cast<int64_t*>(ws + p.offs);
    float* xp = reinterpret_cast<float*>(ws + p.xpad);
    const bool pad = h->cin_pad != C;
    if (pad && total > 0x7fffffff) return g_err.fail(XVEC_ERR_ARG, "too many frames");
    const float* rows = pad ? xp : x_packed;
    // everything is planned before anything is enqueued: layer 5 writes its rows (act5) instead of pooling partials
    LayerPlan lp[XVEC_NUM_TDNN];
    if ((rc = plan_stack(h, rows, h->cin_pad, offs_dev, B, 0, p, dtype, ws, lp, true))) return rc;
    if ((rc = stage_offsets(h, offsets_host, nullptr, B, offs_dev, s))) return rc;
    if (pad) {
        StageTimer t(h, T_PACK, s);
        HIP_TRY(launch_pack_rows(x_packed, nullptr, 1, (int)total, C, h->cin_pad, xp, false, s));
    }
    if (lp[0].mode.src == Src::kRows16) {    // [total, ldx] fp32 -> bf16 hi and lo planes (same row stride in elements)
        StageTimer t(h, T_PACK, s);
        HIP_TRY(launch_pack_rows_split(rows, p.total, h->cin_pad, h->cin_pad, lp[0].a.x_plane_bytes / 2, ws + p.x16, s));
    }
    for (const LayerPlan& l : lp)
        if ((rc = launch_layer(h, l, s))) return rc;
    float* pooled = mode == XVEC_MODE_POOLED ? out : reinterpret_cast<float*>(ws + sp.pooled);
    {
        StageTimer t(h, T_POOL, s);
        const LayerPlan& l5 = lp[XVEC_NUM_TDNN - 1];
        const int n5 = h->geo[4].n_pad;
        const bool b16 = dtype == XVEC_BF16;                 // its layer 5 left relu(z + bias'): BatchNorm goes to the statistics
        PoolSegArgs a;
        memset(&a, 0, sizeof(a));
        a.y = l5.a.Y;
        a.elem = b16 ? 1 : 0;
        a.rows = total - (int64_t)B * XVEC_TOTAL_CONTEXT;
        a.ldy = l5.a.ldy;
        a.C = XVEC_POOL_CHANNELS;
        a.row0 = reinterpret_cast<int64_t*>(ws + sp.seg_row);
        a.n = reinterpret_cast<int32_t*>(ws + sp.seg_n);
        a.n_segments = n_segments;
        a.scale = b16 ? h->vec[4] + n5 : nullptr;
        a.shift = b16 ? h->vec[4] + 2 * n5 : nullptr;
        a.out = pooled;
        HIP_TRY(launch_segment_rows(seg_utt_dev, seg_start_dev, seg_len_dev, n_segments, offs_dev, B, XVEC_TOTAL_CONTEXT,
                                    reinterpret_cast<int64_t*>(ws + sp.seg_row), reinterpret_cast<int32_t*>(ws + sp.seg_n), s));
        HIP_TRY(launch_pool_segments(a, s));
    }
    if (mode == XVEC_MODE_POOLED) return XVEC_OK;
    return segment_layers(h, pooled, (int)n_segments, reinterpret_cast<float*>(ws + sp.seg6), reinterpret_cast<float*>(ws + sp.seg7),
                          reinterpret_cast<float*>(ws + p.actA), (p.actB - p.actA) * 2, mode, dtype, out, s);
}

int xvec_tdnn_layer(xvec_handle* h, int layer, const float* x, int32_t B, int32_t T, int dtype, float* y,
                    void* workspace, size_t workspace_bytes, xvec_stream stream) {
    if (!h || layer < 0 || layer >= XVEC_NUM_TDNN) return g_err.fail(XVEC_ERR_ARG, "bad handle or layer %d", layer);
    const TdnnGeom& g = h->geo[layer];
    if (B < 1 || T <= g.ctx_span) return g_err.fail(XVEC_ERR_ARG, "need B>=1 and T>%d (got B=%d T=%d)", g.ctx_span, B, T);
    Plan p;
    LayerCall c;
    int rc = layer_entry(h, layer, x, y, B, T, dtype, workspace, workspace_bytes, p, c);
    if (rc) return rc;
    DeviceGuard guard;                 // launches go to the handle's device whatever the caller's current one is
    HIP_TRY(guard.enter(h->cfg.device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    const bool b16 = c.mode.prec == Prec::kBf16;
    // The caller gets fp32.  Plain bf16 keeps its bf16 activation, widened with this layer's BatchNorm.  bf16x3 runs the
    // layer as the whole path does where a kernel of its own writes the two bf16 planes the next layer reads (tdnn_first3,
    // tdnn_pp16.hip at its batch sizes) and joins them (layer 5 writes fp32 from the 128x128 kernel: the whole path pools it).
    c.Y = ws + p.act5;
    LayerPlan lp;
    bool planes = false;
    if (c.mode.prec == Prec::kBf16x3 && layer < XVEC_NUM_TDNN - 1) {
        LayerCall cp = c;
        cp.mode.dst = Dst::kAct;
        cp.y_plane = p.rows_alloc * (int64_t)g.n_pad * 2;
        rc = plan_layer(h, cp, lp);
        planes = lp.launch == Launch::kFirst3 || lp.launch == Launch::kPp16;
        if (planes && rc) return rc;
    }
    if (!planes) {
        if (b16) c.mode.dst = Dst::kAct;
        if ((rc = plan_layer(h, c, lp))) return rc;
    }
    if ((rc = stage_layer_input(h, c, lp, x, B, T, p, ws, s)) || (rc = launch_layer(h, lp, s))) return rc;
    const int To = T - g.ctx_span;
    if (planes) {
        HIP_TRY(launch_unpack_rows_split(c.Y, lp.a.y_plane_bytes / 2, g.n_pad, B, To, To, g.cout, y, s));
    } else {
        HIP_TRY(launch_unpack_rows(c.Y, b16, g.n_pad, B, To, To, g.cout, y, s, b16 ? h->vec[layer] + g.n_pad : nullptr,
                                   b16 ? h->vec[layer] + 2 * g.n_pad : nullptr));
    }
    return XVEC_OK;
}

int xvec_tdnn_pool_layer(xvec_handle* h, const float* x, int32_t B, int32_t T, int dtype, float* out, void* workspace,
                         size_t workspace_bytes, xvec_stream stream) {
    const int layer = XVEC_NUM_TDNN - 1;
    if (!h) return g_err.fail(XVEC_ERR_ARG, "null handle");
    const int span = h->geo[layer].ctx_span;
    if (B < 1 || B > kMaxUtts || T <= span) return g_err.fail(XVEC_ERR_ARG, "need 1<=B<=%d and T>%d (got B=%d T=%d)", kMaxUtts, span, B, T);
    Plan p;
    LayerCall c;
    int rc = layer_entry(h, layer, x, out, B, T, dtype, workspace, workspace_bytes, p, c);
    if (rc) return rc;
    DeviceGuard guard;
    HIP_TRY(guard.enter(h->cfg.device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    c.mode.dst = Dst::kPool;
    c.x_rows = 0;
    c.part = reinterpret_cast<float*>(ws + p.part);
    c.part_cnt = reinterpret_cast<int*>(ws + p.part_cnt);
    LayerPlan lp;
    if ((rc = plan_layer(h, c, lp)) || (rc = stage_layer_input(h, c, lp, x, B, T, p, ws, s)) || (rc = launch_layer(h, lp, s)))
        return rc;
    return finalize_pool(h, lp, out, s);
}

int xvec_stat_pool(const float* x, const int32_t* lengths_dev, int32_t B, int32_t T, int32_t C, float* out,
                   xvec_stream stream) {
    if (!x || !out) return g_err.fail(XVEC_ERR_ARG, "null tensor pointer");
    if (B < 1 || T < 1 || C < 1) return g_err.fail(XVEC_ERR_ARG, "B, T, C must be positive");
    if (B > 65535) return g_err.fail(XVEC_ERR_ARG, "B > 65535 not supported by the stand-alone pooling kernel");
    PoolArgs a;
    memset(&a, 0, sizeof(a));
    a.X = x;
    a.out = out;
    a.lengths = lengths_dev;
    a.B = B;
    a.T = T;
    a.C = C;
    HIP_TRY(launch_stat_pool(a, static_cast<hipStream_t>(stream)));
    return XVEC_OK;
}

int xvec_affine(xvec_handle* h, int which, const float* x, int32_t M, int relu, float* y, xvec_stream stream) {
    const int i = aff_index(which);
    if (!h || i < 0) return g_err.fail(XVEC_ERR_ARG, "bad handle or affine id %d", which);
    if (!x || !y || M < 1) return g_err.fail(XVEC_ERR_ARG, "bad x/y/M");
    if (!h->aff_loaded[i]) return g_err.fail(XVEC_ERR_STATE, "affine %d weights not loaded", which);
    DeviceGuard guard;                 // launches go to the handle's device whatever the caller's current one is
    HIP_TRY(guard.enter(h->cfg.device));
    affine_plan::Plan ran;
    HIP_TRY(launch_affine_f32(x, h->affW[i], h->affB[i], y, M, h->affN[i], h->affK[i], relu,
                              static_cast<hipStream_t>(stream), nullptr, 0, nullptr, &ran));
    h->last_aff_form[i] = ran.form;
    h->last_aff_ranges[i] = ran.S;
    return XVEC_OK;
}

int xvec_segment_layer(xvec_handle* h, int which, const float* x, int32_t M, int relu, int dtype, float* y, void* scratch,
                       size_t scratch_bytes, xvec_stream stream) {
    const int i = aff_index(which);
    if (!h || i < 0) return g_err.fail(XVEC_ERR_ARG, "bad handle or affine id %d", which);
    if (!x || !y || M < 1) return g_err.fail(XVEC_ERR_ARG, "bad x/y/M");
    if (dtype != XVEC_F32 && dtype != XVEC_BF16 && dtype != XVEC_BF16X3) return g_err.fail(XVEC_ERR_ARG, "bad dtype %d", dtype);
    if (!scratch && scratch_bytes) return g_err.fail(XVEC_ERR_ARG, "null scratch of %zu bytes", scratch_bytes);
    if (reinterpret_cast<uintptr_t>(scratch) & 15) return g_err.fail(XVEC_ERR_ARG, "scratch is not 16-byte aligned");
    if (!h->aff_loaded[i]) return g_err.fail(XVEC_ERR_STATE, "affine %d weights not loaded", which);
    DeviceGuard guard;                 // launches go to the handle's device whatever the caller's current one is
    HIP_TRY(guard.enter(h->cfg.device));
    return segment_affine(h, i, x, M, relu, dtype, y, static_cast<float*>(scratch), scratch_bytes, static_cast<hipStream_t>(stream));
}

int xvec_get_affine_dispatch(const xvec_handle* h, int* forms, int* ranges, int* n) {
    if (!h || !forms || !ranges || !n) return g_err.fail(XVEC_ERR_ARG, "null argument");
    for (int i = 0; i < 3; ++i) {
        forms[i] = h->last_aff_form[i];
        ranges[i] = h->last_aff_ranges[i];
    }
    *n = 3;
    return XVEC_OK;
}

int xvec_get_dispatch(const xvec_handle* h, int* kernels, int* n) {
    if (!h || !kernels || !n) return g_err.fail(XVEC_ERR_ARG, "null argument");
    for (int i = 0; i < XVEC_NUM_TDNN; ++i) kernels[i] = h->last_kernel[i];
    *n = XVEC_NUM_TDNN;
    return XVEC_OK;
}

int xvec_get_tdnn_launch(const xvec_handle* h, int* threads, int* blocks, int* n) {
    if (!h || !threads || !blocks || !n) return g_err.fail(XVEC_ERR_ARG, "null argument");
    for (int i = 0; i < XVEC_NUM_TDNN; ++i) {
        threads[i] = h->last_threads[i];
        blocks[i] = h->last_blocks[i];
    }
    *n = XVEC_NUM_TDNN;
    return XVEC_OK;
}

int xvec_get_tdnn_form(const xvec_handle* h, int* forms, int* n) {
    if (!h || !forms || !n) return g_err.fail(XVEC_ERR_ARG, "null argument");
    for (int i = 0; i < XVEC_NUM_TDNN; ++i) forms[i] = h->last_form[i];
    *n = XVEC_NUM_TDNN;
    return XVEC_OK;
}

int xvec_get_tdnn_operands(const xvec_handle* h, int* operands, int* n) {
    if (!h || !operands || !n) return g_err.fail(XVEC_ERR_ARG, "null argument");
    for (int i = 0; i < XVEC_NUM_TDNN; ++i) operands[i] = h->last_operands[i];
    *n = XVEC_NUM_TDNN;
    return XVEC_OK;
}

int xvec_set_profiling(xvec_handle* h, int on) {
    if (!h) return g_err.fail(XVEC_ERR_ARG, "null handle");
    h->profiling = on != 0;
    for (int i = 0; i < T_COUNT; ++i) h->ev_used[i] = false;
    return XVEC_OK;
}

int xvec_get_timings(xvec_handle* h, float* ms, int* n) {
    if (!h || !ms || !n) return g_err.fail(XVEC_ERR_ARG, "null argument");
    for (int i = 0; i < T_COUNT; ++i) {
        ms[i] = 0.f;
        if (h->ev_used[i]) {
            HIP_TRY(hipEventSynchronize(h->ev1[i]));
            HIP_TRY(hipEventElapsedTime(&ms[i], h->ev0[i], h->ev1[i]));
        }
    }
    *n = T_COUNT;
    return XVEC_OK;
}

}  // extern "C"
