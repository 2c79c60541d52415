// The tables of the MFCC front end (mfcc.hip), built on the host: the package's filterbank and DCT x lifter in double
// precision, the twiddles of both kernels, and the layouts the nfft-512 kernel reads them in (MFMA B fragments, the banded
// filterbank, its gather table).  Standard C++17 over std::vector, no HIP: xvec_mfcc_create uploads the result, and
// tests/abi/mfcc_tables_dump.cpp writes it out for tests/test_mfcc_tables.py on a machine without a GPU.
//
// Everything sits in the unnamed namespace (and fft512 inside it) that mfcc.hip's kernels live in: the layout constants
// below are the kernels' own.  Each including translation unit gets its own copy.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/xvec_hip.h"

namespace {

constexpr int kMaxNfft = 4096;
constexpr int kThreads = 256;

namespace fft512 {

constexpr int kTile = 16;                   // frames per block pass
constexpr int kEx = 576;                    // complex slots of a wave's exchange region (8 x 72)
constexpr int kPS = 264;                    // floats per row of the power-spectrum tile (256 + 8) and of the log-mel tile: row strides of 8 mod 64
constexpr int kLS = 40;                     // dwords put the sixteen lanes of a ds_read_b128 service group (rows r, lane quads q: 16-byte
                                            // fragments at 4 q) on sixteen distinct 4-bank windows (260 / 36: one 2-way conflict per group)
constexpr int kMaxItems = 5;                // (filter tile, bin group) products per wave: 20 per block (the default filterbank has 18)
// The power rows of a wave's SECOND pair of frames live in its own exchange region (idle from that pair's last exchange to the
// next tile's first), its partial sums behind them; only the first pairs' eight rows have storage of their own: 30 016 bytes a
// block, five blocks on a CU (round 6; sixteen rows of their own were 38 464 bytes, four blocks).
constexpr int kExRow = 16;                  // floats: the rows in wave w's region start at 16 w + 4: with the row stride (8 mod 64) the
constexpr int kExRow0 = 4;                  // eight rows of the array sit on bank offsets 0, 8, ..., 56 and these eight on 4, 12, ..., 60
constexpr int kExPart = 592;                // floats: the partial sums (2 x 64 lanes x 4) behind the rows (3 x 16 + 4 + 2 x 264 = 580)
static_assert(3 * kExRow + kExRow0 + 2 * kPS <= kExPart && kExPart + 512 <= 2 * kEx && kExPart % 4 == 0 && kExRow0 % 4 == 0,
              "layout of an exchange region");
constexpr int kLdsFloats = 4 * kEx * 2 + (kTile / 2) * kPS + kTile * kLS + 2 * kTile + 2 * 56;
// ---- the banded filterbank (round 6).  A bin carries weight for two neighbouring triangles, the dense form multiplies it
// with sixteen: 18 products of 16 x 16 x 16 per tile, 32 cycles of the matrix pipe per 16 x 16 x 4 step, 640 cycles per wave
// and tile -- a fifth of a SIMD's busy time.  v_mfma_f32_4x4x1_16b_f32 is SIXTEEN independent 4 x 4 x 1 products (8 cycles):
// block 4 fq + s takes frames 4 fq .. + 3 (rows) of ONE bin and the bin's weights for FOUR neighbouring filters (columns).
// The host cuts the bins into at most 15 GROUPS of at most 20 consecutive bins whose filters fit one window of four (a .. a + 3);
// wave w owns groups 4 w .. 4 w + 3, SLOT s of its instructions is group 4 w + s, instruction n the group's bin n: 20
// instructions of 8 cycles per wave and tile, every lane ends with a group's [4 frames] x one filter, nothing to add across
// lanes.  The summing threads gather per filter the (at most eight) groups that hold it, in bin order; an absent entry points
// at group 15, whose weights are all zero.
constexpr int kBandN = 20;                  // instructions per tile and wave = bins a group's lanes read
constexpr int kBandCap = 19;                // bins of a group that may carry weight: one bin of play, so that the four groups of a wave
                                            // can start their reads on four different residues mod 4 -- with the sixteen rows on bank
                                            // offsets 0, 4, ..., 60 the 64 lanes of a read then fall on 64 different banks
constexpr int kBandGroups = 15;             // (+ the all-zero group 15)
constexpr int kBandGat = 8;                 // groups a filter can collect from
constexpr int kBandLdsFloats = kLdsFloats + kBandGat * 32;   // + the gather table
static_assert(kBandLdsFloats * 4 <= 32 * 1024, "five blocks per CU");

}  // namespace fft512

// Every table of a plan in one blob of floats (ints stored bit for bit), and where each one starts.
struct MfccTables {
    std::vector<float> blob;
    // the general kernel's LDS image: twiddles per pass | dctl[numcep][nfilt|1] | fb_w[fb_nnz] | fb_lo[nfilt] | fb_off[nfilt+1]
    int tw_off, dctl_off, fbw_off, fblo_off, fboff_off, table_floats;
    // the nfft-512 kernel's tables behind it (MfccDev in mfcc.hip documents their shapes); f_band == -1: no banded form
    int f_tw1, f_tw2, f_fb, f_dct, f_band, f_gat;
    int f_lo0, f_n0, f_lo1, f_n1, f_gat_n;
    int frame_len, frame_step, log2n, nbins;
    bool fast;    // nfft == 512, nfilt <= 32, numcep <= 32: fft512::mfcc512_kernel
};

// The message of a failed build_mfcc_tables (the caller copies it into its error channel).
struct ErrorText {
    const char* text = "";
    int fail(int code, const char* msg) {
        text = msg;
        return code;
    }
};

inline int round_half_up(double v) { return (int)std::floor(v + 0.5); }   // sigproc.round_half_up for v >= 0

// non-zero weights only: filter j covers bins [lo_j, lo_j + len_j), its weights are w[off_j .. off_(j+1))
struct SparseFilterbank {
    std::vector<float> w;
    std::vector<int> lo, off;
};

// python_speech_features.base.get_filterbanks, in double
inline SparseFilterbank mel_filterbank(const xvec_mfcc_cfg& cfg) {
    const int nfft = cfg.nfft, nbins = nfft / 2 + 1, nfilt = cfg.nfilt;
    const double high = cfg.highfreq > 0 ? cfg.highfreq : cfg.samplerate / 2.0, low = cfg.lowfreq;
    auto hz2mel = [](double hz) { return 2595.0 * std::log10(1.0 + hz / 700.0); };
    auto mel2hz = [](double mel) { return 700.0 * (std::pow(10.0, mel / 2595.0) - 1.0); };
    std::vector<double> bins(nfilt + 2);
    for (int i = 0; i < nfilt + 2; ++i) {
        const double mel = hz2mel(low) + (hz2mel(high) - hz2mel(low)) * i / (nfilt + 1);
        bins[i] = std::floor((nfft + 1) * mel2hz(mel) / cfg.samplerate);
    }
    SparseFilterbank fb;
    fb.lo.resize(nfilt);
    fb.off.resize(nfilt + 1);
    for (int j = 0; j < nfilt; ++j) {
        const int b0 = std::min((int)bins[j], nbins), b1 = std::min((int)bins[j + 1], nbins),
                  b2 = std::min((int)bins[j + 2], nbins);
        fb.lo[j] = b0;
        fb.off[j] = (int)fb.w.size();
        for (int i = b0; i < b1; ++i) fb.w.push_back((float)((i - bins[j]) / (bins[j + 1] - bins[j])));
        for (int i = b1; i < b2; ++i) fb.w.push_back((float)((bins[j + 2] - i) / (bins[j + 2] - bins[j + 1])));
    }
    fb.off[nfilt] = (int)fb.w.size();
    return fb;
}

// scipy dct(type=2, norm='ortho') rows times base.lifter: [numcep][nfilt | 1]
inline std::vector<float> dct_lifter_rows(const xvec_mfcc_cfg& cfg) {
    const int nfilt = cfg.nfilt, dct_ld = nfilt | 1;
    std::vector<float> dctl((size_t)cfg.numcep * dct_ld, 0.f);
    for (int k = 0; k < cfg.numcep; ++k) {
        const double scale = std::sqrt((k == 0 ? 1.0 : 2.0) / nfilt);
        const double lift = cfg.ceplifter > 0 ? 1.0 + (cfg.ceplifter / 2.0) * std::sin(M_PI * k / cfg.ceplifter) : 1.0;
        for (int m = 0; m < nfilt; ++m)
            dctl[(size_t)k * dct_ld + m] = (float)(std::cos(M_PI * k * (2 * m + 1) / (2.0 * nfilt)) * scale * lift);
    }
    return dctl;
}

// twiddles W_M^j = exp(-2 pi i j / M), grouped per pass of the kernel: for h = 1, 4, 16, ...
// records {W_2h^j, W_4h^j, W_4h^(j+h)}, j < h; then, for odd log2(nfft), W_N^j, j < N/2
inline std::vector<float> pass_twiddles(int log2n) {
    std::vector<float> tw;
    auto push_w = [&](int j, int M) {
        tw.push_back((float)std::cos(2.0 * M_PI * j / M));
        tw.push_back((float)(-std::sin(2.0 * M_PI * j / M)));
    };
    int st = 0;
    for (; st + 1 < log2n; st += 2) {
        const int h = 1 << st;
        for (int j = 0; j < h; ++j) {
            push_w(j, 2 * h);
            push_w(j, 4 * h);
            push_w(j + h, 4 * h);
        }
    }
    if (st < log2n)
        for (int j = 0; j < (1 << log2n) / 2; ++j) push_w(j, 1 << log2n);
    return tw;
}

// the nfft-512 kernel's step 1: [7][64] complex, W_512^(lane * k), k = 1..7
inline std::vector<float> fft512_lane_twiddles() {
    std::vector<float> tw;
    for (int k = 1; k < 8; ++k)
        for (int l = 0; l < 64; ++l) {
            tw.push_back((float)std::cos(2.0 * M_PI * (l * k) / 512.0));
            tw.push_back((float)(-std::sin(2.0 * M_PI * (l * k) / 512.0)));
        }
    return tw;
}

// ... and its step 2: [7][8] complex, W_64^(c * k)
inline std::vector<float> fft512_step2_twiddles() {
    std::vector<float> tw;
    for (int k = 1; k < 8; ++k)
        for (int c = 0; c < 8; ++c) {
            tw.push_back((float)std::cos(2.0 * M_PI * (c * k) / 64.0) * 0.015625f);   // (x 2^-6: fft512, kTwoM6)
            tw.push_back((float)(-std::sin(2.0 * M_PI * (c * k) / 64.0)) * 0.015625f);
        }
    return tw;
}

// dense filterbank [32][256] (bin 256 never carries a weight: the last edge is exclusive)
inline std::vector<float> dense_filterbank(const SparseFilterbank& fb) {
    std::vector<float> dense(32 * 256, 0.f);
    for (int j = 0; j < (int)fb.lo.size(); ++j)
        for (int k = 0; k < fb.off[j + 1] - fb.off[j]; ++k)
            if (fb.lo[j] + k < 256) dense[j * 256 + fb.lo[j] + k] = 2.f * fb.w[fb.off[j] + k];   // (x 2: the kernel's power rows are halves, kTwoM6)
    return dense;
}

// -> B fragments of v_mfma_f32_16x16x4_f32: lane l of product (tile t, group g) holds FB[16t + (l & 15)][16g + 4(l >> 4) + j];
// g_lo / g_n: the bin groups of tile t with a non-zero weight, [g_lo[t], g_lo[t] + g_n[t])
inline std::vector<float> filterbank_fragments(const std::vector<float>& dense, int g_lo[2], int g_n[2]) {
    std::vector<float> frag;
    int g_hi[2] = {0, 0};
    g_lo[0] = g_lo[1] = 16;
    for (int t = 0; t < 2; ++t)
        for (int g = 0; g < 16; ++g)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 4; ++j) {
                    const float w = dense[(16 * t + (l & 15)) * 256 + 16 * g + 4 * (l >> 4) + j];
                    frag.push_back(w);
                    if (w != 0.f) {
                        g_lo[t] = std::min(g_lo[t], g);
                        g_hi[t] = std::max(g_hi[t], g + 1);
                    }
                }
    for (int t = 0; t < 2; ++t) {
        if (g_hi[t] <= g_lo[t]) g_lo[t] = g_hi[t] = 0;
        g_n[t] = g_hi[t] - g_lo[t];
    }
    return frag;
}

// the DCT x lifter rows, zero padded to 32 x 32, as B fragments: [2 cepstrum tiles][2 filter groups][64 lanes][4]
inline std::vector<float> dct_fragments(const std::vector<float>& dctl, int numcep, int nfilt) {
    std::vector<float> frag;
    for (int t = 0; t < 2; ++t)
        for (int g = 0; g < 2; ++g)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 4; ++j) {
                    const int c = 16 * t + (l & 15), m = 16 * g + 4 * (l >> 4) + j;
                    frag.push_back(c < numcep && m < nfilt ? dctl[(size_t)c * (nfilt | 1) + m] : 0.f);
                }
    return frag;
}

// ---- the banded form (fft512::kBand*): groups of consecutive bins whose filters fit a window of four
struct BandGroups {
    int k[16] = {}, cnt[16] = {}, a[16] = {}, n = 0;   // first bin, bins, first filter (group 15 stays empty: all-zero weights)
    bool ok = true;                                    // false: more than kBandGroups groups, or one bin wider than a window
};

inline BandGroups band_groups(const std::vector<float>& dense) {
    using namespace fft512;
    int fmin[256], fmax[256];
    for (int k = 0; k < 256; ++k) {
        fmin[k] = 32;
        fmax[k] = -1;
        for (int j = 0; j < 32; ++j)
            if (dense[j * 256 + k] != 0.f) {
                fmin[k] = std::min(fmin[k], j);
                fmax[k] = std::max(fmax[k], j);
            }
    }
    BandGroups gr;
    for (int k = 0; k < 256 && gr.ok;) {
        if (gr.n == kBandGroups) { gr.ok = false; break; }
        int a = -1, cnt = 0;
        const int k0 = k;
        while (k < 256 && cnt < kBandCap) {
            if (fmax[k] >= 0) {                            // (a bin without weight joins any group)
                if (a < 0) a = std::min(fmin[k], 28);
                if (fmax[k] > a + 3) break;
            }
            ++k;
            ++cnt;
        }
        if (cnt == 0) { gr.ok = false; break; }            // one bin wider than a window
        gr.k[gr.n] = k0;
        gr.cnt[gr.n] = cnt;
        gr.a[gr.n++] = a < 0 ? 0 : a;
    }
    return gr;
}

// where the partial sums of group g, frame quad 0, filter column j sit (bytes from the start of the block's LDS):
// wave g >> 2 writes lane 16 fq + 4 (g & 3) + j
inline int band_part_byte(int g, int j) {
    using namespace fft512;
    return ((g >> 2) * 2 * kEx + kExPart) * 4 + ((g & 3) * 4 + j) * 16;
}

// the gather table [kBandGat][32]: per filter, the partial sums of the groups that hold a weight of it, in group order;
// gat_n: the longest list.  False: a filter in more than kBandGat groups.
inline bool band_gather_table(const std::vector<float>& dense, const BandGroups& gr, std::vector<int>& gat, int& gat_n) {
    using namespace fft512;
    gat.assign(kBandGat * 32, band_part_byte(15, 0));      // absent: a column of the all-zero group
    gat_n = 0;
    for (int f = 0; f < 32; ++f) {
        int e = 0;
        for (int g = 0; g < gr.n; ++g) {
            if (f < gr.a[g] || f > gr.a[g] + 3) continue;
            bool any = false;
            for (int k = gr.k[g]; k < gr.k[g] + gr.cnt[g]; ++k) any = any || dense[f * 256 + k] != 0.f;
            if (!any) continue;
            if (e == kBandGat) {
                gat_n = kBandGat;
                return false;
            }
            gat[e++ * 32 + f] = band_part_byte(g, f - gr.a[g]);
        }
        gat_n = std::max(gat_n, e);
    }
    return true;
}

// first bin a group's lanes read: anywhere in [k + cnt - 20, k] (bins in front of the group carry weight 0), inside
// the row, and -- where that leaves a choice -- on a residue mod 4 no earlier group of the wave reads on
inline void band_read_starts(const BandGroups& gr, int k_rd[16]) {
    using namespace fft512;
    for (int w = 0; w < 4; ++w) {
        bool used[4] = {false, false, false, false};
        for (int sl = 0; sl < 4; ++sl) {
            const int g = 4 * w + sl;
            const int hi_k = g < gr.n ? std::min(gr.k[g], 256 - kBandN) : 256 - kBandN;
            const int lo_k = g < gr.n ? std::max(0, gr.k[g] + gr.cnt[g] - kBandN) : 0;
            int pick = hi_k;
            for (int kk = hi_k; kk >= lo_k; --kk)
                if (!used[kk & 3]) { pick = kk; break; }
            used[pick & 3] = true;
            k_rd[g] = pick;
        }
    }
}

// [4 waves][5][64 lanes][4]: 20 weights per lane (instruction n = 4 q + c); behind them [4 waves][64 lanes] LDS byte offsets
inline std::vector<float> band_weights_and_offsets(const std::vector<float>& dense, const BandGroups& gr, const int k_rd[16]) {
    using namespace fft512;
    std::vector<float> band;
    for (int w = 0; w < 4; ++w)
        for (int q5 = 0; q5 < 5; ++q5)
            for (int l = 0; l < 64; ++l)
                for (int c = 0; c < 4; ++c) {          // weight of instruction n = 4 q5 + c: bin n of group 4 w + slot
                    const int g = 4 * w + ((l >> 2) & 3), t = l & 3, kk = k_rd[g] + 4 * q5 + c;
                    const bool live = g < gr.n && kk >= gr.k[g] && kk < gr.k[g] + gr.cnt[g];
                    band.push_back(live ? dense[(gr.a[g] + t) * 256 + kk] : 0.f);
                }
    for (int w = 0; w < 4; ++w)                        // LDS byte address of frame 4 fq + t at the group's first bin
        for (int l = 0; l < 64; ++l) {
            const int fq = l >> 4, g = 4 * w + ((l >> 2) & 3), t = l & 3;
            const int rowf = (t >> 1) ? fq * (2 * kEx + kExRow) + kExRow0 + (t & 1) * kPS : 4 * kEx * 2 + (2 * fq + (t & 1)) * kPS;
            const int byte = (rowf + k_rd[g]) * 4;
            float fv;
            memcpy(&fv, &byte, 4);
            band.push_back(fv);
        }
    return band;
}

inline int append(std::vector<float>& blob, const std::vector<float>& v) {
    const int o = (int)blob.size();
    blob.insert(blob.end(), v.begin(), v.end());
    return o;
}
inline int append(std::vector<float>& blob, const std::vector<int>& v) {   // (ints stored bit-for-bit in the float array)
    const int o = (int)blob.size();
    for (int x : v) {
        float fv;
        memcpy(&fv, &x, 4);
        blob.push_back(fv);
    }
    return o;
}
inline int align_to(std::vector<float>& blob, int floats) {
    while (blob.size() % floats) blob.push_back(0.f);
    return (int)blob.size();
}

// tables of the nfft == 512 kernel, after the LDS image (16-byte aligned); allow_banded == false keeps the dense products for
// a filterbank the banded form can hold (tests and A/B timing)
inline void append_fft512_tables(const xvec_mfcc_cfg& cfg, const SparseFilterbank& fb, const std::vector<float>& dctl,
                                 bool allow_banded, MfccTables& t) {
    t.f_tw1 = align_to(t.blob, 4);
    append(t.blob, fft512_lane_twiddles());
    t.f_tw2 = append(t.blob, fft512_step2_twiddles());
    const std::vector<float> dense = dense_filterbank(fb);
    int g_lo[2], g_n[2];
    t.f_fb = append(t.blob, filterbank_fragments(dense, g_lo, g_n));
    t.f_lo0 = g_lo[0];
    t.f_n0 = g_n[0];
    t.f_lo1 = g_lo[1];
    t.f_n1 = g_n[1];
    if (t.f_n0 + t.f_n1 > 4 * fft512::kMaxItems) t.fast = false;   // an unusually dense filterbank
    t.f_dct = append(t.blob, dct_fragments(dctl, cfg.numcep, cfg.nfilt));
    const BandGroups gr = band_groups(dense);
    std::vector<int> gat;
    if (!(gr.ok && band_gather_table(dense, gr, gat, t.f_gat_n) && allow_banded)) return;
    int k_rd[16];
    band_read_starts(gr, k_rd);
    t.f_band = align_to(t.blob, 4);
    append(t.blob, band_weights_and_offsets(dense, gr, k_rd));
    t.f_gat = append(t.blob, gat);
}

// Checks the configuration (everything that needs no device) and builds every table of its plan.
inline int build_mfcc_tables(const xvec_mfcc_cfg& cfg, bool allow_banded, MfccTables& t, ErrorText& err) {
    const int nfft = cfg.nfft;
    int log2n = 0;
    while ((1 << log2n) < nfft) ++log2n;
    if (nfft < 64 || nfft > kMaxNfft || (1 << log2n) != nfft) return err.fail(XVEC_ERR_ARG, "nfft must be a power of two in [64, 4096]");
    if (cfg.samplerate < 1 || cfg.nfilt < 1 || cfg.nfilt > kThreads || cfg.nfilt > nfft / 2 + 1 ||
        cfg.numcep < 1 || cfg.numcep > cfg.nfilt)
        return err.fail(XVEC_ERR_ARG, "need 1 <= numcep <= nfilt <= min(256, nfft/2+1) and a positive sample rate");
    t = MfccTables();
    t.f_band = -1;
    t.frame_len = round_half_up((double)cfg.winlen * cfg.samplerate);
    t.frame_step = round_half_up((double)cfg.winstep * cfg.samplerate);
    if (t.frame_len < 1 || t.frame_step < 1) return err.fail(XVEC_ERR_ARG, "window length/step too small");
    t.log2n = log2n;
    t.nbins = nfft / 2 + 1;
    const SparseFilterbank fb = mel_filterbank(cfg);
    const std::vector<float> dctl = dct_lifter_rows(cfg);
    // one blob: twiddle | dctl | fb_w | fb_lo | fb_off
    t.tw_off = append(t.blob, pass_twiddles(log2n));
    t.dctl_off = append(t.blob, dctl);
    t.fbw_off = append(t.blob, fb.w);
    t.fblo_off = append(t.blob, fb.lo);
    t.fboff_off = append(t.blob, fb.off);
    t.table_floats = align_to(t.blob, 2);                // keep the per-wave regions 8-byte aligned
    t.fast = (nfft == 512 && cfg.nfilt <= 32 && cfg.numcep <= 32);
    if (t.fast) append_fft512_tables(cfg, fb, dctl, allow_banded, t);
    return XVEC_OK;
}

}  // namespace
