// MXFP4 (OCP e2m1 codes, e8m0 block scales) on v_mfma_scale_f32_32x32x64_f8f6f4 cbsz:4 blgp:4, gfx950: operand, nibble and
// scale lane maps with exact data, and the sustained MFMA-only rate next to the e4m3 form of the same instruction.
//   build: hipcc --offload-arch=gfx950 -O3 mxfp4_mfma.hip -o mxfp4_mfma        output kept in profiles/r16_mxfp4_mfma.txt
// include/rtv_hip_mxfp4.h's layout statement rests on what this prints.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef __attribute__((ext_vector_type(8))) int v8i;
typedef __attribute__((ext_vector_type(4))) int v4i;
typedef __attribute__((ext_vector_type(16))) float f32x16;

__device__ __forceinline__ v8i widen(v4i x) { return __builtin_shufflevector(x, x, 0, 1, 2, 3, -1, -1, -1, -1); }

// Hypothesis under test: lane l holds row l & 31 and the 32 consecutive K elements 32 * (l >> 5) .. + 32 of the 64-deep step as 16
// packed bytes (element 2j in the low nibble of byte j), and its scale byte (the byte of the scale register that opsel selects)
// applies to exactly those 32 elements.  sA / sB: [32 rows][2 blocks] dwords whose byte OPSEL is the block's scale; the other three
// bytes hold decoys.
template <int OPA, int OPB>
__global__ void probe(const unsigned char* A /*[32][32 bytes]*/, const unsigned char* B, const unsigned* sA, const unsigned* sB,
                      float* D /*[32][32]*/) {
  const int l = threadIdx.x, r = l & 31, g = l >> 5;
  const v4i a = *(const v4i*)(A + r * 32 + g * 16), b = *(const v4i*)(B + r * 32 + g * 16);
  f32x16 c = {0};
  c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(widen(a), widen(b), c, 4, 4, OPA, (int)sA[r * 2 + g], OPB, (int)sB[r * 2 + g]);
  // C/D layout of 32x32 MFMAs: col = lane & 31, row = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5)
  for (int i = 0; i < 16; ++i) D[((i & 3) + 8 * (i >> 2) + 4 * g) * 32 + r] = c[i];
}

template <int FP4>
__global__ __launch_bounds__(256) void rate(float* out, int iters) {
  v8i a[2], b[2];
  unsigned h = (blockIdx.x * 256 + threadIdx.x) * 2654435761u + 12345u;
  for (int s = 0; s < 2; ++s)
    for (int i = 0; i < 8; ++i) {
      h = h * 1664525u + 1013904223u; a[s][i] = (int)(h & 0x77777777u);   // e4m3 bytes without NaN patterns; any nibble is a valid e2m1
      h = h * 1664525u + 1013904223u; b[s][i] = (int)(h & 0x77777777u);
    }
  f32x16 acc[4];
  for (int n = 0; n < 4; ++n) for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
  const int sc = 0x7f7e7f7e + (int)(threadIdx.x & 1);
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        if (FP4) acc[n] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[(u + n) & 1], b[u & 1], acc[n], 4, 4, 0, sc, 1, sc);
        else acc[n] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[(u + n) & 1], b[u & 1], acc[n], 0, 0, 0, 0, 0, 0);
      }
  }
  float s = 0.f;
  for (int n = 0; n < 4; ++n) for (int r = 0; r < 16; ++r) s += acc[n][r];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

static float e2m1(int c) {
  static const float mag[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};
  return (c & 8) ? -mag[c & 7] : mag[c & 7];
}
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

template <int OPA, int OPB>
static int run_probe(const char* what, bool identity) {
  std::vector<unsigned char> A(32 * 32), B(32 * 32);
  std::vector<unsigned> sA(64), sB(64);
  std::vector<int> eA(64), eB(64);
  srand(7 + OPA * 4 + OPB);
  for (auto& x : A) x = (unsigned char)(rand() & 0xff);
  for (auto& x : B) x = (unsigned char)(rand() & 0xff);
  if (identity)   // A = identity-like: row m holds one 1.0 (code 2) at k = m and k = 32 + ((m + 5) & 31), zero elsewhere
    for (int m = 0; m < 32; ++m) {
      for (int j = 0; j < 32; ++j) A[m * 32 + j] = 0;
      const int k0 = m, k1 = 32 + ((m + 5) & 31);
      A[m * 32 + k0 / 2] |= (unsigned char)(2 << (4 * (k0 & 1)));
      A[m * 32 + k1 / 2] |= (unsigned char)(2 << (4 * (k1 & 1)));
    }
  for (int i = 0; i < 64; ++i) {   // distinct exponent per (row, lane half); decoy bytes differ from the live one
    eA[i] = (i * 5) % 13 - 6;
    eB[i] = (i * 7) % 11 - 5;
    unsigned da = 0x5a6b7c8du + i, db = 0x91a2b3c4u + 3 * i;
    sA[i] = (da & ~(0xffu << (8 * OPA))) | ((unsigned)(eA[i] + 127) << (8 * OPA));
    sB[i] = (db & ~(0xffu << (8 * OPB))) | ((unsigned)(eB[i] + 127) << (8 * OPB));
  }
  unsigned char *dA, *dB; unsigned *dsA, *dsB; float* dD;
  CK(hipMalloc(&dA, 1024)); CK(hipMalloc(&dB, 1024)); CK(hipMalloc(&dsA, 256)); CK(hipMalloc(&dsB, 256)); CK(hipMalloc(&dD, 4096));
  CK(hipMemcpy(dA, A.data(), 1024, hipMemcpyHostToDevice)); CK(hipMemcpy(dB, B.data(), 1024, hipMemcpyHostToDevice));
  CK(hipMemcpy(dsA, sA.data(), 256, hipMemcpyHostToDevice)); CK(hipMemcpy(dsB, sB.data(), 256, hipMemcpyHostToDevice));
  probe<OPA, OPB><<<1, 64>>>(dA, dB, dsA, dsB, dD);
  CK(hipDeviceSynchronize());
  std::vector<float> D(1024);
  CK(hipMemcpy(D.data(), dD, 4096, hipMemcpyDeviceToHost));
  // hypotheses: nibble order (low first / high first) x orientation (D[m][n] / D[n][m]) x scales (per lane half / lane half 0's for
  // the whole row / none)
  const char* nn[2] = {"low nibble first", "high nibble first"};
  const char* on[2] = {"D[m][n]", "D[n][m]"};
  const char* sn[3] = {"scale of the lane's own 32-block", "lane half 0's scale for all 64", "scales ignored"};
  int exact = 0;
  for (int nib = 0; nib < 2; ++nib)
    for (int ori = 0; ori < 2; ++ori)
      for (int sm = 0; sm < 3; ++sm) {
        double err = 0, ref_max = 0;
        for (int m = 0; m < 32; ++m)
          for (int n = 0; n < 32; ++n) {
            double r = 0;
            for (int k = 0; k < 64; ++k) {
              const int sh = 4 * ((k & 1) ^ nib), blk = k >> 5;
              const double a = e2m1((A[m * 32 + k / 2] >> sh) & 15), b = e2m1((B[n * 32 + k / 2] >> sh) & 15);
              const int e = sm == 0 ? eA[m * 2 + blk] + eB[n * 2 + blk] : sm == 1 ? eA[m * 2] + eB[n * 2] : 0;
              r += ldexp(a * b, e);
            }
            err = fmax(err, fabs((ori ? D[n * 32 + m] : D[m * 32 + n]) - r));
            ref_max = fmax(ref_max, fabs(r));
          }
        if (err == 0) {
          printf("probe %s opsel a=%d b=%d: EXACT under [%s, %s, %s] (ref max %.6g)\n", what, OPA, OPB, nn[nib], on[ori], sn[sm], ref_max);
          ++exact;
        }
      }
  if (!exact) printf("probe %s opsel a=%d b=%d: NO hypothesis is exact\n", what, OPA, OPB);
  CK(hipFree(dA)); CK(hipFree(dB)); CK(hipFree(dsA)); CK(hipFree(dsB)); CK(hipFree(dD));
  return 0;
}

int main() {
  if (run_probe<0, 0>("identity-like A, random B", true)) return 1;
  if (run_probe<0, 0>("random A, random B", false)) return 1;
  if (run_probe<1, 2>("random A, random B", false)) return 1;
  if (run_probe<3, 1>("random A, random B", false)) return 1;
  if (run_probe<2, 3>("identity-like A, random B", true)) return 1;
  // ---- rates
  float* out; CK(hipMalloc(&out, 512 * 256 * 4));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  for (int fp4 : {1, 0}) {
    const int iters = 50000;
    for (int rep = 0; rep < 2; ++rep) {
      CK(hipEventRecord(e0));
      if (fp4) rate<1><<<512, 256>>>(out, iters); else rate<0><<<512, 256>>>(out, iters);
      CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
      float ms; CK(hipEventElapsedTime(&ms, e0, e1));
      const double flops = 512.0 * 4 * iters * 16 * 2.0 * 32 * 32 * 64;
      printf("mfma 32x32x64 %s: %.2f ms  %.1f TF/s (random operands, 2 waves/SIMD)\n", fp4 ? "e2m1 + e8m0 scales" : "e4m3, no scales", ms,
             flops / ms / 1e9);
    }
  }
  return 0;
}
