// How often does v_mfma_f32_32x32x16_bf16 round inside one instruction?  (decides whether the
// bf16_split3 form of the fp32 1-tap layers may keep its six products in one accumulator.)
//
// One wave, one MFMA per case, C given.  Every product of two bf16 values is exact in fp32 and the
// 16 products plus C sum exactly in fp64 here (exponents within 40 binades), so each output can be set
// against models of the instruction's adder:
//   once  - the exact sum of C and all 16 products, rounded once to fp32 (round to nearest even)
//   seqK  - C + p_0 + ... + p_15 rounded to fp32 after every product, k ascending (an fmaf chain)
//   gG    - products summed exactly in groups of G consecutive k, each group then added to the fp32
//           running sum with one rounding (G = 2, 4, 8)
//   trunc - the exact sum truncated toward zero once
// Directed cases first (a row of 1 and fifteen 2^-25 against ones: exact 1 + 4 ulp, per-product rounding 1),
// then random cases with large cancellation, where the models disagree on a good share of outputs.
//
// Build + run: hipcc --offload-arch=gfx950 -O2 -o /tmp/mfma_rnd profiles/experiments/mfma_bf16_rounding.hip && /tmp/mfma_rnd
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// A[32][16], B[16][32], C[32][32] per case (row-major), D[32][32] out
__global__ __launch_bounds__(64) void probe(const __bf16* A, const __bf16* B, const float* C, float* D, int n_cases) {
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    for (int t = 0; t < n_cases; ++t) {
        const __bf16* a = A + t * 512;
        const __bf16* b = B + t * 512;
        bf16x8 av, bv;
        for (int j = 0; j < 8; ++j) {
            av[j] = a[r * 16 + 8 * h + j];        // A operand: row r, k = 8h + j
            bv[j] = b[(8 * h + j) * 32 + r];      // B operand: column r, k = 8h + j
        }
        f32x16 acc;
        for (int e = 0; e < 16; ++e) acc[e] = C[t * 1024 + ((e & 3) + 8 * (e >> 2) + 4 * h) * 32 + r];
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc, 0, 0, 0);
        for (int e = 0; e < 16; ++e) D[t * 1024 + ((e & 3) + 8 * (e >> 2) + 4 * h) * 32 + r] = acc[e];
    }
}

static uint16_t bf_bits(float f) {   // f must be representable in bf16
    uint32_t u;
    memcpy(&u, &f, 4);
    return (uint16_t)(u >> 16);
}
static float bf_val(uint16_t b) {
    uint32_t u = (uint32_t)b << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static uint32_t rng = 12345u;
static uint32_t nxt() { rng = rng * 1664525u + 1013904223u; return rng >> 8; }

int main() {
    const int n_dir = 6, n_rand = 64, n = n_dir + n_rand;
    std::vector<uint16_t> A(n * 512), B(n * 512);
    std::vector<float> C(n * 1024, 0.f), D(n * 1024);
    // directed: case 0..3: row of [1 at position p, fifteen 2^-25] x ones, C = 0 (p = 0, 7, 8, 15);
    // case 4: fifteen 2^-25 and a 0, C = 1;  case 5: 1 at 0, one 2^-24 + 2^-25.. pattern: k odd 2^-24, k even>0 2^-26
    const float one = 1.f, s25 = ldexpf(1.f, -25), s24 = ldexpf(1.f, -24), s26 = ldexpf(1.f, -26);
    for (int t = 0; t < n_dir; ++t)
        for (int i = 0; i < 32; ++i)
            for (int k = 0; k < 16; ++k) {
                float v;
                if (t < 4) { const int p = t == 0 ? 0 : t == 1 ? 7 : t == 2 ? 8 : 15; v = k == p ? one : s25; }
                else if (t == 4) { v = k == 15 ? 0.f : s25; C[t * 1024 + i * 32 + 0] = 0.f; }
                else v = k == 0 ? one : (k & 1) ? s24 : s26;
                A[t * 512 + i * 16 + k] = bf_bits(v);
                B[t * 512 + k * 32 + i] = bf_bits(one);
            }
    for (int e = 0; e < 1024; ++e) C[4 * 1024 + e] = 1.f;
    // random: products of magnitude 2^-20..2^0 with random signs, C = +-(0..4): heavy cancellation
    for (int t = n_dir; t < n; ++t) {
        for (int i = 0; i < 512; ++i) {
            const float m = 1.f + (float)(nxt() & 127) / 128.f;
            const int ex = -(int)(nxt() % 11);
            A[t * 512 + i] = bf_bits(((nxt() & 1) ? -1.f : 1.f) * ldexpf(m, ex));
            const float m2 = 1.f + (float)(nxt() & 127) / 128.f;
            B[t * 512 + i] = bf_bits(((nxt() & 1) ? -1.f : 1.f) * ldexpf(m2, -(int)(nxt() % 11)));
        }
        for (int i = 0; i < 1024; ++i) C[t * 1024 + i] = ((nxt() & 1) ? -1.f : 1.f) * (float)(nxt() % 4096) / 1024.f;
    }
    __bf16 *dA, *dB;
    float *dC, *dD;
    if (hipMalloc(&dA, A.size() * 2) || hipMalloc(&dB, B.size() * 2) || hipMalloc(&dC, C.size() * 4) || hipMalloc(&dD, D.size() * 4)) return 1;
    (void)hipMemcpy(dA, A.data(), A.size() * 2, hipMemcpyHostToDevice);
    (void)hipMemcpy(dB, B.data(), B.size() * 2, hipMemcpyHostToDevice);
    (void)hipMemcpy(dC, C.data(), C.size() * 4, hipMemcpyHostToDevice);
    probe<<<1, 64>>>(dA, dB, dC, dD, n);
    if (hipDeviceSynchronize() != hipSuccess) { printf("kernel failed\n"); return 1; }
    (void)hipMemcpy(D.data(), dD, D.size() * 4, hipMemcpyDeviceToHost);

    const char* names[] = {"once", "seqK", "g2", "g4", "g8", "trunc"};
    long match[2][6] = {};
    long total[2] = {};
    for (int t = 0; t < n; ++t)
        for (int i = 0; i < 32; ++i)
            for (int j = 0; j < 32; ++j) {
                double p[16];
                for (int k = 0; k < 16; ++k) p[k] = (double)bf_val(A[t * 512 + i * 16 + k]) * (double)bf_val(B[t * 512 + k * 32 + j]);
                const float c = C[t * 1024 + i * 32 + j], d = D[t * 1024 + i * 32 + j];
                double ex = c;
                for (int k = 0; k < 16; ++k) ex += p[k];
                float m[6];
                m[0] = (float)ex;
                float s = c;
                for (int k = 0; k < 16; ++k) s = (float)((double)s + p[k]);
                m[1] = s;
                const int gs[3] = {2, 4, 8};
                for (int gi = 0; gi < 3; ++gi) {
                    float sg = c;
                    for (int k0 = 0; k0 < 16; k0 += gs[gi]) {
                        double g = 0;
                        for (int k = k0; k < k0 + gs[gi]; ++k) g += p[k];
                        sg = (float)((double)sg + g);
                    }
                    m[2 + gi] = sg;
                }
                float tz = (float)ex;
                if (fabs((double)tz) > fabs(ex)) tz = nextafterf(tz, 0.f);
                m[5] = tz;
                const int kind = t < n_dir ? 0 : 1;
                ++total[kind];
                for (int q = 0; q < 6; ++q) match[kind][q] += (m[q] == d);
                if (t < n_dir && i == 0 && j == 0)
                    printf("directed case %d: got 1 + %.4g ulp  (once %.4g, seqK %.4g, g4 %.4g, g8 %.4g, trunc %.4g ulp)\n", t,
                           (d - 1.0) / ldexp(1.0, -23), (m[0] - 1.0) / ldexp(1.0, -23), (m[1] - 1.0) / ldexp(1.0, -23),
                           (m[3] - 1.0) / ldexp(1.0, -23), (m[4] - 1.0) / ldexp(1.0, -23), (m[5] - 1.0) / ldexp(1.0, -23));
            }
    for (int kind = 0; kind < 2; ++kind) {
        printf("%s outputs (%ld): matches", kind ? "random" : "directed", total[kind]);
        for (int q = 0; q < 6; ++q) printf("  %s %.4f", names[q], (double)match[kind][q] / total[kind]);
        printf("\n");
    }
    return 0;
}
