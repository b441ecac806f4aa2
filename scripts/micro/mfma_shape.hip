// Which bf16 matrix instruction sustains the higher rate under the power cap: v_mfma_f32_32x32x16_bf16 or v_mfma_f32_16x16x32_bf16?
// Both shapes compute the SAME 64 x 64 output tile per wave, 64 deep per loop iteration (16 MFMAs of the large shape, 32 of the
// small one, the same 64 accumulator and 64 fragment registers), so FLOPs per iteration are equal and only the instruction differs.
//
//   *_reg: operands stay in registers; the timed loop is matrix instructions and loop control, nothing else.
//   *_lds: every operand is re-read from LDS by ds_read_b128 before each use (16 reads per iteration, 8 behind the MFMAs of each
//          32-deep half, into the fragment set of the other half) + one s_waitcnt per half: the operand traffic of a GEMM main loop.
//
// Accumulators (a[0:63]) and fragments (a[64:127]) are accumulation registers named literally in inline asm, as in csrc/gemm5.hip:
// the compiler has no value to move.  (mfma_peak16.hip left its sixteen f32x4 accumulators to the compiler, which shuffled them
// through accumulation registers: 96 v_accvgpr moves per 32 MFMAs - that loop measured VALU issue, not the instruction.)
// scripts/micro/mfma_shape_audit.sh checks the loop bodies statically.
//   build: hipcc --offload-arch=gfx950 -O3 mfma_shape.hip -o mfma_shape        run: ./mfma_shape [iters=100000] [warm_ms=1000]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {
constexpr int ACC0 = 0, FRAG0 = 64;   // a[0:63] accumulators, a[64:127] fragments: [half][A0..A3 | B0..B3] x 4 registers
// every register the asm owns: the clobber list makes the kernel descriptor allocate them.  A clobber does not reserve a register
// across statements, so the audit also counts, over the WHOLE kernel (set-up and read-out included), instructions outside
// ASMSTART / ASMEND that name an accumulation register: hipcc must place no value of its own there (compiler_acc_refs 0).
#define MS_CLOBBER \
  "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", "a10", "a11", "a12", "a13", "a14", "a15", "a16", "a17", \
  "a18", "a19", "a20", "a21", "a22", "a23", "a24", "a25", "a26", "a27", "a28", "a29", "a30", "a31", "a32", "a33", "a34", \
  "a35", "a36", "a37", "a38", "a39", "a40", "a41", "a42", "a43", "a44", "a45", "a46", "a47", "a48", "a49", "a50", "a51", \
  "a52", "a53", "a54", "a55", "a56", "a57", "a58", "a59", "a60", "a61", "a62", "a63", "a64", "a65", "a66", "a67", "a68", \
  "a69", "a70", "a71", "a72", "a73", "a74", "a75", "a76", "a77", "a78", "a79", "a80", "a81", "a82", "a83", "a84", "a85", \
  "a86", "a87", "a88", "a89", "a90", "a91", "a92", "a93", "a94", "a95", "a96", "a97", "a98", "a99", "a100", "a101", \
  "a102", "a103", "a104", "a105", "a106", "a107", "a108", "a109", "a110", "a111", "a112", "a113", "a114", "a115", "a116", \
  "a117", "a118", "a119", "a120", "a121", "a122", "a123", "a124", "a125", "a126", "a127"

template <int ACC, int A, int B>
__device__ __forceinline__ void mfma32() {
  asm volatile("v_mfma_f32_32x32x16_bf16 a[%c0:%c1], a[%c2:%c3], a[%c4:%c5], a[%c0:%c1]" ::"n"(ACC), "n"(ACC + 15), "n"(A), "n"(A + 3), "n"(B),
               "n"(B + 3));
}
template <int ACC, int A, int B>
__device__ __forceinline__ void mfma16() {
  asm volatile("v_mfma_f32_16x16x32_bf16 a[%c0:%c1], a[%c2:%c3], a[%c4:%c5], a[%c0:%c1]" ::"n"(ACC), "n"(ACC + 3), "n"(A), "n"(A + 3), "n"(B),
               "n"(B + 3));
}
template <int DST, int OFF>
__device__ __forceinline__ void lds_read128_a(uint32_t addr) {
  asm volatile("ds_read_b128 a[%c1:%c2], %0 offset:%3" ::"v"(addr), "n"(DST), "n"(DST + 3), "n"(OFF));
}
template <int DST>
__device__ __forceinline__ void acc_write(float v) {
  asm volatile("v_accvgpr_write_b32 a[%c1], %0" ::"v"(v), "n"(DST));
}
template <int SRC>
__device__ __forceinline__ float acc_read() {
  float r;
  asm volatile("v_accvgpr_read_b32 %0, a[%c1]" : "=v"(r) : "n"(SRC));
  return r;
}
template <int I>
struct IC { static constexpr int value = I; };
template <int B, int E, class F>
__device__ __forceinline__ void sfor(F&& f) {
  if constexpr (B < E) {
    f(IC<B>{});
    sfor<B + 1, E>(f);
  }
}

__device__ __forceinline__ float rnd(unsigned& h, int random, float c) {
  h = h * 1664525u + 1013904223u;
  return random ? (((h >> 8) & 0xffff) / 65536.f - 0.5f) * 3.f : c;
}
__device__ __forceinline__ uint32_t pack2(float a, float b) {
  __bf16 x = (__bf16)a, y = (__bf16)b;
  return (uint32_t) * (unsigned short*)&x | ((uint32_t) * (unsigned short*)&y << 16);
}

// MFMA n of the 32-deep half H.  Fragment f of a half: registers FRAG0 + 32 H + 4 f; f = 0..3 the A operand, 4..7 the B operand.
//   32x32x16:  8 per half = [ks 2][mb 2][nb 2]: A fragment 2 mb + ks, B fragment 4 + 2 nb + ks, accumulator block 2 mb + nb (16 registers)
//   16x16x32: 16 per half =       [mb 4][nb 4]: A fragment mb,        B fragment 4 + nb,        accumulator block 4 mb + nb ( 4 registers)
template <int SHAPE, int H, int n>
__device__ __forceinline__ void mfma_n() {
  constexpr int F = FRAG0 + 32 * H;
  if constexpr (SHAPE == 32) {
    constexpr int ks = n >> 2, mb = (n >> 1) & 1, nb = n & 1;
    mfma32<ACC0 + 16 * (2 * mb + nb), F + 4 * (2 * mb + ks), F + 4 * (4 + 2 * nb + ks)>();
  } else {
    constexpr int mb = n >> 2, nb = n & 3;
    mfma16<ACC0 + 4 * (4 * mb + nb), F + 4 * mb, F + 4 * (4 + nb)>();
  }
}

template <int SHAPE, bool LDS>
__device__ __forceinline__ void body(float* out, int iters, long long* clk, int random) {
  constexpr int PER_HALF = SHAPE == 32 ? 8 : 16;     // MFMAs per 32-deep half
  constexpr int READ_EVERY = PER_HALF / 8;           // one ds_read_b128 behind every MFMA (32x32x16) / every second one (16x16x32)
  __shared__ __attribute__((aligned(16))) uint32_t lds[LDS ? 16 * 256 : 4];   // 16 fragments x 64 lanes x 16 bytes
  unsigned h = (blockIdx.x * 256 + threadIdx.x) * 2654435761u + 12345u;
  asm volatile("" ::: MS_CLOBBER);
  if constexpr (LDS) {
    for (int i = 0; i < 16; ++i) {
      const float c = (i & 4) ? 0.5f : 1.0f;
      lds[i * 256 + threadIdx.x] = pack2(rnd(h, random, c), rnd(h, random, c));
    }
    __syncthreads();
  }
  const uint32_t addr = (uint32_t)(size_t)(__attribute__((address_space(3))) uint32_t*)lds + (threadIdx.x & 63) * 16;
  sfor<0, 64>([&](auto ic) __attribute__((always_inline)) { acc_write<ACC0 + decltype(ic)::value>(0.f); });
  if constexpr (LDS) {
    sfor<0, 16>([&](auto ic) __attribute__((always_inline)) { lds_read128_a<FRAG0 + 4 * decltype(ic)::value, 1024 * decltype(ic)::value>(addr); });
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  } else {
    sfor<0, 64>([&](auto ic) __attribute__((always_inline)) {
      const float c = (decltype(ic)::value & 16) ? 0.5f : 1.0f;
      acc_write<FRAG0 + decltype(ic)::value>(__uint_as_float(pack2(rnd(h, random, c), rnd(h, random, c))));
    });
  }
  asm volatile("s_nop 7");
  __builtin_amdgcn_sched_barrier(0);
  const long long t0 = __builtin_amdgcn_s_memrealtime();
  const long long c0 = __builtin_amdgcn_s_memtime();
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll 1
  for (int it = 0; it < iters; ++it) {
    asm volatile("; MFMA_SHAPE_BODY_BEGIN");
    sfor<0, 2>([&](auto hc) __attribute__((always_inline)) {
      constexpr int H = decltype(hc)::value;
      sfor<0, PER_HALF>([&](auto nc) __attribute__((always_inline)) {
        constexpr int n = decltype(nc)::value;
        mfma_n<SHAPE, H, n>();
        if constexpr (LDS && n % READ_EVERY == 0) {   // fragment n / READ_EVERY of the OTHER half (its last use: the half before this one)
          constexpr int f = n / READ_EVERY, G = H ^ 1;
          lds_read128_a<FRAG0 + 32 * G + 4 * f, 1024 * (8 * G + f)>(addr);
        }
      });
      if constexpr (LDS) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    });
    asm volatile("; MFMA_SHAPE_BODY_END");
  }
  __builtin_amdgcn_sched_barrier(0);
  const long long c1 = __builtin_amdgcn_s_memtime();
  const long long t1 = __builtin_amdgcn_s_memrealtime();
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_nop 15\n\ts_nop 7");
  float s = 0.f;
  sfor<0, 64>([&](auto ic) __attribute__((always_inline)) { s += acc_read<ACC0 + decltype(ic)::value>(); });
  out[blockIdx.x * 256 + threadIdx.x] = s;
  if (threadIdx.x == 0) {   // stamps: a buffer of their own
    clk[blockIdx.x * 2] = c1 - c0;
    clk[blockIdx.x * 2 + 1] = t1 - t0;
  }
}
}  // namespace

extern "C" __global__ __launch_bounds__(256) void mfma32_reg(float* o, int n, long long* c, int r) { body<32, false>(o, n, c, r); }
extern "C" __global__ __launch_bounds__(256) void mfma16_reg(float* o, int n, long long* c, int r) { body<16, false>(o, n, c, r); }
extern "C" __global__ __launch_bounds__(256) void mfma32_lds(float* o, int n, long long* c, int r) { body<32, true>(o, n, c, r); }
extern "C" __global__ __launch_bounds__(256) void mfma16_lds(float* o, int n, long long* c, int r) { body<16, true>(o, n, c, r); }

#define CK(x)                                                                      \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess) {                                                        \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                      \
      return 1;                                                                    \
    }                                                                              \
  } while (0)

int main(int argc, char** argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 100000;
  const double warm_ms = argc > 2 ? atof(argv[2]) : 1000.0;
  constexpr int MAXB = 512;
  float* out;
  long long* clk;
  CK(hipMalloc(&out, (size_t)MAXB * 256 * 4));
  CK(hipMalloc(&clk, (size_t)MAXB * 16));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  std::vector<long long> hc(MAXB * 2);
  std::vector<float> ho((size_t)MAXB * 256);
  auto launch = [&](int shape, int lds, int blocks, int random) {
    if (lds) (shape == 32 ? mfma32_lds : mfma16_lds)<<<blocks, 256>>>(out, iters, clk, random);
    else (shape == 32 ? mfma32_reg : mfma16_reg)<<<blocks, 256>>>(out, iters, clk, random);
  };
  printf("# 64x64 output tile per wave, 64 deep per iteration; iters %d; each line: >= %.0f ms of back-to-back launches, then the median of 3\n",
         iters, warm_ms);
  for (int lds = 0; lds < 2; ++lds)
    for (int wps = 1; wps <= 2; ++wps)
      for (int random = 1; random >= 0; --random)
        for (int alt = 0; alt < 4; ++alt) {   // 32, 16, 32, 16: the repeat shows the spread
          const int shape = (alt & 1) ? 16 : 32, blocks = 256 * wps;
          const int per_iter = shape == 32 ? 16 : 32;
          float ms = 0.f;
          double warmed = 0.0;
          while (warmed < warm_ms) {
            CK(hipEventRecord(e0));
            launch(shape, lds, blocks, random);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            CK(hipEventElapsedTime(&ms, e0, e1));
            warmed += ms;
          }
          double t[3], cyc[3], mhz[3];
          for (int rep = 0; rep < 3; ++rep) {
            CK(hipEventRecord(e0));
            launch(shape, lds, blocks, random);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            CK(hipEventElapsedTime(&ms, e0, e1));
            CK(hipMemcpy(hc.data(), clk, (size_t)blocks * 16, hipMemcpyDeviceToHost));
            std::vector<double> cy(blocks), cl(blocks);
            for (int b = 0; b < blocks; ++b) {
              cy[b] = (double)hc[2 * b] / ((double)iters * per_iter);
              cl[b] = (double)hc[2 * b] / ((double)hc[2 * b + 1] / 100.0);
            }
            std::nth_element(cy.begin(), cy.begin() + blocks / 2, cy.end());
            std::nth_element(cl.begin(), cl.begin() + blocks / 2, cl.end());
            t[rep] = ms, cyc[rep] = cy[blocks / 2], mhz[rep] = cl[blocks / 2];
          }
          std::sort(t, t + 3), std::sort(cyc, cyc + 3), std::sort(mhz, mhz + 3);
          CK(hipMemcpy(ho.data(), out, (size_t)blocks * 256 * 4, hipMemcpyDeviceToHost));
          double sum = 0.0;
          for (size_t i = 0; i < (size_t)blocks * 256; ++i) sum += ho[i];
          const double flops = (double)blocks * 4 * iters * 2.0 * 64 * 64 * 64;
          printf("%s %s waves/SIMD=%d operands=%-8s  %8.3f ms  %7.1f TF/s  wave cycles/MFMA %6.2f (per 32x32x16 equivalent %6.2f)  in-kernel clock %4.0f MHz  checksum %.6g\n",
                 shape == 32 ? "32x32x16" : "16x16x32", lds ? "lds" : "reg", wps, random ? "random" : "constant", t[1], flops / t[1] / 1e9, cyc[1],
                 cyc[1] * per_iter / 16.0, mhz[1], sum);
          fflush(stdout);
        }
  return 0;
}
