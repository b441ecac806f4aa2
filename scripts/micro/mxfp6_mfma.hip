// MXFP6 (OCP e2m3 codes, e8m0 block scales) on v_mfma_scale_f32_32x32x64_f8f6f4 cbsz:2 blgp:2, gfx950: the operand image (which
// bits of a lane's six registers hold which element), the scale lane map, both with exact data, and the sustained MFMA-only rate
// next to the e2m1 and e4m3 forms of the same instruction.
//   build: hipcc --offload-arch=gfx950 -O3 mxfp6_mfma.hip -o mxfp6_mfma        output kept in profiles/r17_mxfp6_mfma.txt
// include/rtv_hip_mxfp6.h's layout statement rests on what this prints.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
typedef __attribute__((ext_vector_type(8))) int v8i;
typedef __attribute__((ext_vector_type(16))) float f32x16;

// Hypothesis under test: lane l holds row l & 31 and the 32 consecutive K elements 32 * (l >> 5) .. + 32 of the 64-deep step as one
// little-endian 192-bit string in operand registers 0-5 (element j at bits [6 j, 6 j + 6)), and its scale byte (the byte of the
// scale register that opsel selects) applies to exactly those 32 elements.  A / B: [32 rows][2 blocks][24 bytes]; sA / sB:
// [32 rows][2 blocks] dwords whose byte OPSEL is the block's scale, the other three bytes hold decoys.  Registers 6 and 7 of the
// builtin's 8-register type carry garbage on purpose: the instruction must not read them.
template <int OPA, int OPB>
__global__ void probe(const unsigned* A, const unsigned* B, const unsigned* sA, const unsigned* sB, float* D /*[32][32]*/) {
  const int l = threadIdx.x, r = l & 31, g = l >> 5;
  v8i a, b;
  for (int i = 0; i < 6; ++i) {
    a[i] = (int)A[(r * 2 + g) * 6 + i];
    b[i] = (int)B[(r * 2 + g) * 6 + i];
  }
  a[6] = 0x7bdef7bd + l; a[7] = ~l; b[6] = 0x3def7bde - l; b[7] = l * 77;
  f32x16 c = {0};
  c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 2, 2, OPA, (int)sA[r * 2 + g], OPB, (int)sB[r * 2 + g]);
  // C/D layout of 32x32 MFMAs: col = lane & 31, row = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5)
  for (int i = 0; i < 16; ++i) D[((i & 3) + 8 * (i >> 2) + 4 * g) * 32 + r] = c[i];
}

template <int FMT>   // 4: e2m1, 2: e2m3, 0: e4m3 without scales
__global__ __launch_bounds__(256) void rate(float* out, int iters) {
  v8i a[2], b[2];
  unsigned h = (blockIdx.x * 256 + threadIdx.x) * 2654435761u + 12345u;
  for (int s = 0; s < 2; ++s)
    for (int i = 0; i < 8; ++i) {
      h = h * 1664525u + 1013904223u; a[s][i] = (int)(h & 0x77777777u);   // e4m3 bytes without NaN patterns; any bits are valid e2m1 / e2m3
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
        if (FMT == 4) acc[n] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[(u + n) & 1], b[u & 1], acc[n], 4, 4, 0, sc, 1, sc);
        else if (FMT == 2) acc[n] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[(u + n) & 1], b[u & 1], acc[n], 2, 2, 0, sc, 1, sc);
        else acc[n] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[(u + n) & 1], b[u & 1], acc[n], 0, 0, 0, 0, 0, 0);
      }
  }
  float s = 0.f;
  for (int n = 0; n < 4; ++n) for (int r = 0; r < 16; ++r) s += acc[n][r];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

static double e2m3(int c) {
  const int ex = (c >> 3) & 3, m = c & 7;
  const double mag = ex == 0 ? m / 8.0 : (1 + m / 8.0) * (double)(1 << (ex - 1));
  return (c & 32) ? -mag : mag;
}
// code of element j of a 24-byte block under packing hypothesis `pk`
//   0: one little-endian 192-bit string, element j at bits [6 j, 6 j + 6), a code's mantissa in its low bits
//   1: the same 6-bit fields with the four codes of every 3-byte group in the opposite order - a permutation of the elements of a
//      block, applied to both operands: it cannot change a dot product, so it must come out exact wherever 0 does (it says that
//      the order of the elements inside a block is not observable, and not material)
//   2: the fields of 0 with the bits of every code reversed (sign in bit 0)
//   3: the string read from the top bit of every byte (fields that straddle bytes differently)
static int code_at(const unsigned char* blk, int j, int pk) {
  const int bit = pk == 1 ? 24 * (j / 4) + 6 * (3 - j % 4) : 6 * j;
  unsigned v = 0;
  for (int i = 0; i < 6; ++i) {
    const int b = bit + i;
    const unsigned x = pk == 3 ? (blk[b >> 3] >> (7 - (b & 7))) & 1u : (blk[b >> 3] >> (b & 7)) & 1u;
    v |= x << (pk == 2 ? 5 - i : i);
  }
  return (int)v;
}
static void put_code(unsigned char* blk, int j, int code) {   // packing 0
  const int bit = 6 * j;
  for (int i = 0; i < 6; ++i) {
    blk[(bit + i) >> 3] &= (unsigned char)~(1u << ((bit + i) & 7));
    blk[(bit + i) >> 3] |= (unsigned char)(((code >> i) & 1) << ((bit + i) & 7));
  }
}
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

template <int OPA, int OPB>
static int run_probe(const char* what, bool identity) {
  std::vector<unsigned char> A(32 * 48), B(32 * 48);
  std::vector<unsigned> sA(64), sB(64);
  std::vector<int> eA(64), eB(64);
  srand(7 + OPA * 4 + OPB);
  for (auto& x : A) x = (unsigned char)(rand() & 0xff);
  for (auto& x : B) x = (unsigned char)(rand() & 0xff);
  if (identity)   // A = identity-like: row m holds one 1.0 (code 8) at k = m and one 1.5 (code 12) at k = 32 + ((m + 5) & 31), zero elsewhere
    for (int m = 0; m < 32; ++m) {
      memset(&A[m * 48], 0, 48);
      put_code(&A[m * 48], m, 8);
      put_code(&A[m * 48 + 24], (m + 5) & 31, 12);
    }
  for (int i = 0; i < 64; ++i) {   // distinct exponent per (row, lane half); decoy bytes differ from the live one
    // identity-like A: an output is two terms, exact whatever the exponents.  Random A: terms are multiples of 2^-6 2^(ea + eb) and
    // 64 of them sum to at most 64 * 56.25 * 2^(ea + eb); with both exponents in {-1, 0, 1} every partial sum is a multiple of 2^-8
    // below 2^14, exact in fp32 in any order - what is printed is then the map and not the accumulator's rounding
    eA[i] = identity ? (i * 5) % 13 - 6 : (i * 5) % 3 - 1;
    eB[i] = identity ? (i * 7) % 11 - 5 : (i * 7 + 1) % 3 - 1;
    unsigned da = 0x5a6b7c8du + i, db = 0x91a2b3c4u + 3 * i;
    sA[i] = (da & ~(0xffu << (8 * OPA))) | ((unsigned)(eA[i] + 127) << (8 * OPA));
    sB[i] = (db & ~(0xffu << (8 * OPB))) | ((unsigned)(eB[i] + 127) << (8 * OPB));
  }
  unsigned char *dA, *dB; unsigned *dsA, *dsB; float* dD;
  CK(hipMalloc(&dA, 1536)); CK(hipMalloc(&dB, 1536)); CK(hipMalloc(&dsA, 256)); CK(hipMalloc(&dsB, 256)); CK(hipMalloc(&dD, 4096));
  CK(hipMemcpy(dA, A.data(), 1536, hipMemcpyHostToDevice)); CK(hipMemcpy(dB, B.data(), 1536, hipMemcpyHostToDevice));
  CK(hipMemcpy(dsA, sA.data(), 256, hipMemcpyHostToDevice)); CK(hipMemcpy(dsB, sB.data(), 256, hipMemcpyHostToDevice));
  probe<OPA, OPB><<<1, 64>>>((const unsigned*)dA, (const unsigned*)dB, dsA, dsB, dD);
  CK(hipDeviceSynchronize());
  std::vector<float> D(1024);
  CK(hipMemcpy(D.data(), dD, 4096, hipMemcpyDeviceToHost));
  // hypotheses: packing (above: 4) x orientation (D[m][n] / D[n][m]) x scales (per lane half / lane half 0's for the whole row / none)
  const char* pn[4] = {"little-endian 192-bit string, element j at bit 6 j", "elements of a 3-byte group reversed", "code bits reversed",
                       "bytes read from the top bit"};
  const char* on[2] = {"D[m][n]", "D[n][m]"};
  const char* sn[3] = {"scale of the lane's own 32-block", "lane half 0's scale for all 64", "scales ignored"};
  int exact = 0;
  for (int pk = 0; pk < 4; ++pk)
    for (int ori = 0; ori < 2; ++ori)
      for (int sm = 0; sm < 3; ++sm) {
        double err = 0, ref_max = 0;
        for (int m = 0; m < 32; ++m)
          for (int n = 0; n < 32; ++n) {
            double r = 0;
            for (int k = 0; k < 64; ++k) {
              const int blk = k >> 5;
              const double a = e2m3(code_at(&A[m * 48 + blk * 24], k & 31, pk)), b = e2m3(code_at(&B[n * 48 + blk * 24], k & 31, pk));
              const int e = sm == 0 ? eA[m * 2 + blk] + eB[n * 2 + blk] : sm == 1 ? eA[m * 2] + eB[n * 2] : 0;
              r += ldexp(a * b, e);
            }
            err = fmax(err, fabs((ori ? D[n * 32 + m] : D[m * 32 + n]) - r));
            ref_max = fmax(ref_max, fabs(r));
          }
        if (err == 0) {
          printf("probe %s opsel a=%d b=%d: EXACT under [%s, %s, %s] (ref max %.6g)\n", what, OPA, OPB, pn[pk], on[ori], sn[sm], ref_max);
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
  for (int rep = 0; rep < 2; ++rep)
    for (int fmt : {2, 4, 0}) {
      const int iters = 50000;
      CK(hipEventRecord(e0));
      if (fmt == 2) rate<2><<<512, 256>>>(out, iters); else if (fmt == 4) rate<4><<<512, 256>>>(out, iters); else rate<0><<<512, 256>>>(out, iters);
      CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
      float ms; CK(hipEventElapsedTime(&ms, e0, e1));
      const double flops = 512.0 * 4 * iters * 16 * 2.0 * 32 * 32 * 64;
      printf("mfma 32x32x64 %s: %.2f ms  %.1f TF/s (random operands, 2 waves/SIMD)\n",
             fmt == 2 ? "e2m3 + e8m0 scales" : fmt == 4 ? "e2m1 + e8m0 scales" : "e4m3, no scales", ms, flops / ms / 1e9);
    }
  return 0;
}
