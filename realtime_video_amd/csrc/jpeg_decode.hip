// Frame input side, second half: a camera's JPEG file -> rgb8 on the device (include/rtv_hip_jpeg_decode.h states the streams
// accepted and the arithmetic).  The host parses the marker segments (jpeg_decode_core.h, jd::parse); two launches per call:
//
//   entropy   one workgroup of 1024 threads = one frame.  The scan is cut into subsequences of a fixed number of bits, one per
//             thread (at most 1024: the length is raised for long scans).  Round 0: every thread decodes its subsequence from a
//             guessed state (start of an MCU) and leaves the state in which it crossed the subsequence's end - bit position, zigzag
//             index, block slot - in LDS.  Round r: a thread whose predecessor's exit state differs from the state it started
//             from decodes again from that state.  Huffman streams resynchronise within a few symbols, so a few rounds settle
//             everything; the loop ends when a round changes nothing, and since subsequence 0 starts from the true state and
//             round r settles subsequence r at the latest, after at most as many rounds as there are subsequences - the serial
//             decode, the bound.  The barrier is __syncthreads(); nothing spins and nothing is shared between workgroups.  Then
//             a scan of (markers crossed, blocks completed) gives every subsequence its first block's index, a final pass writes
//             the coefficients (de-zigzagged, int16) to their blocks in the arena, and the DC terms are rebuilt by a segmented
//             scan of the differences per component (segments = restart intervals).  A restart marker needs no guess: behind it
//             the state is known, and its MCU index follows from the count of the markers in front of it.
//   pixels    one workgroup = 8 MCUs of one MCU row of one frame: dequantisation and the islow IDCT of its luma blocks and of the
//             chroma blocks it needs (with one block of context on each side where the chroma is subsampled) into LDS sample
//             planes, then fancy upsampling and colour conversion out of LDS, rgb8 cropped to the true size.
//
// The state machine, the bit reader (0xFF00 unstuffing happens there) and every bounds check are in jpeg_decode_core.h, which the
// host check program compiles too: what a damaged file does to them is found out on the CPU.
#include "rtv_common.h"
#include "rtv_internal.h"
#include "jpeg_decode_core.h"

namespace rtv {
namespace {

constexpr int ENT_THREADS = jd::MAX_SUBSEQ;
constexpr int PX_MCUS = 8;                    // MCUs of one pixel workgroup
constexpr int PX_THREADS = 256;

__constant__ uint8_t kNatural[64] = JD_NATURAL_ORDER;

struct FrameArg {
  const uint8_t* frame;       // descriptor plus file
  int16_t* coef;              // the frame's coefficient planes in the arena
  uint8_t* out;               // rgb8
  jd::Geom g;
  uint32_t select;            // jd::Tables::select
};
struct DecodeArgs {           // travels by value with the launch
  FrameArg f[RTV_FRAMES_MAX];
};

// exclusive scan of jd::Counts over the workgroup's 1024 threads with jd::combine; *total = the combination of all
__device__ __forceinline__ jd::Counts scan_counts(jd::Counts v, jd::Counts* lds /* [16] */, jd::Counts* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  jd::Counts s = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    jd::Counts o;
    o.c = __shfl_up(s.c, d);
    o.n = __shfl_up(s.n, d);
    if (lane >= d) s = jd::combine(o, s);
  }
  __syncthreads();                      // the previous call's readers are done with lds
  if (lane == 63) lds[wave] = s;
  __syncthreads();
  jd::Counts base = {0, 0}, tot = {0, 0};
  for (int w = 0; w < ENT_THREADS / 64; ++w) {
    const jd::Counts x = lds[w];
    if (w < wave) base = jd::combine(base, x);
    tot = jd::combine(tot, x);
  }
  *total = tot;
  jd::Counts prev;                      // the inclusive value of the lane in front
  prev.c = __shfl_up(s.c, 1);
  prev.n = __shfl_up(s.n, 1);
  return lane ? jd::combine(base, prev) : base;
}

__global__ void __launch_bounds__(ENT_THREADS) jpeg_entropy_decode_kernel(const DecodeArgs a, int subseq_bits, int* __restrict__ status,
                                                                           int* __restrict__ rounds) {
  __shared__ jd::Huff huff[4];
  __shared__ uint8_t natural[64];
  __shared__ jd::State exits[ENT_THREADS];
  __shared__ jd::Counts scan_lds[ENT_THREADS / 64];
  __shared__ int first_err, status_lds, reached_lds;
  const int tid = threadIdx.x, t = blockIdx.x;
  const FrameArg& fa = a.f[t];
  const jd::Geom g = fa.g;
  {
    const uint32_t* src = (const uint32_t*)(fa.frame + offsetof(rtv_jpeg_desc, huff));
    uint32_t* dst = (uint32_t*)huff;
    for (int i = tid; i < 4 * RTV_JPEG_HUFF_WORDS; i += ENT_THREADS) dst[i] = src[i];
    if (tid < 64) natural[tid] = kNatural[tid];
    if (tid == 0) first_err = ENT_THREADS, status_lds = 0, reached_lds = 0;
    uint4* z = (uint4*)fa.coef;                                  // a block is 128 bytes: the planes are whole uint4s
    const int nz = g.coef_elems() / 8;
    for (int i = tid; i < nz; i += ENT_THREADS) z[i] = uint4{0u, 0u, 0u, 0u};
  }
  jd::Tables T;
  T.huff = huff, T.natural = natural;
  T.select = fa.select;
  const uint8_t* scan = fa.frame + sizeof(rtv_jpeg_desc) + g.scan_offset;
  const uint32_t L = (uint32_t)jd::effective_subseq_bits(subseq_bits, g.scan_bytes);
  const uint32_t nbits = (uint32_t)g.scan_bytes * 8u;
  const int nsub = nbits ? (int)((nbits + L - 1) / L) : 1;       // <= ENT_THREADS by the choice of L
  const bool live = tid < nsub;
  const uint32_t end_bit = tid == nsub - 1 ? jd::END_BIT - 1u : (uint32_t)(tid + 1) * L;
  __syncthreads();

  jd::State entry = tid == 0 ? jd::State{0u, 0u} : jd::guessed_state(scan, (uint32_t)g.scan_bytes, (uint32_t)tid * L);
  jd::State ex = entry;
  jd::Counts cnt = {0, 0};
  int err = 0;
  jd::NullSink none;
  if (live) ex = jd::decode_subsequence<false>(T, g, scan, entry, end_bit, &cnt, &err, none);
  exits[tid] = ex;
  int round = 1;
  for (; round <= nsub; ++round) {                               // the bound: round r settles subsequence r at the latest
    __syncthreads();
    jd::State want = entry;
    if (live && tid > 0) want = exits[tid - 1];
    const bool changed = !(want == entry);
    if (!__syncthreads_or(changed ? 1 : 0)) break;
    if (changed) {
      entry = want;
      ex = jd::decode_subsequence<false>(T, g, scan, entry, end_bit, &cnt, &err, none);
      exits[tid] = ex;
    }
  }
  if (live && err) atomicMin(&first_err, tid);
  jd::Counts total;
  const jd::Counts base = scan_counts(live ? cnt : jd::Counts{0, 0}, scan_lds, &total);   // its barriers publish first_err too
  const int stop = first_err;
  if (live && tid <= stop) {                                     // the final pass: nothing behind the first error is written
    jd::CoefSink sink = {fa.coef, natural, g, base, 0, 0};
    jd::Counts again;
    int e;
    jd::decode_subsequence<true>(T, g, scan, entry, end_bit, &again, &e, sink);
    if (sink.status | e) atomicOr(&status_lds, sink.status | e);
    atomicMax(&reached_lds, sink.reached);
  }
  __syncthreads();
  const int reached = reached_lds;

  // DC terms: pred += difference along the scan order of each component, from 0 at every restart interval's first MCU
  const int mcus = g.mcu_cols * g.mcu_rows, per = (mcus + ENT_THREADS - 1) / ENT_THREADS;
  const int m0 = min(tid * per, mcus), m1 = min(m0 + per, mcus);
  for (int c = 0; c < g.ncomp; ++c) {
    const int slot0 = c ? g.hs * g.vs + c - 1 : 0, slots = c ? 1 : g.hs * g.vs;
    jd::Counts mine = {0, 0};
    for (int m = m0; m < m1; ++m) {
      if (g.ri > 0 && m % g.ri == 0) mine = jd::Counts{mine.c + 1, 0};
      for (int s = slot0; s < slot0 + slots; ++s)
        if (m * g.bpm + s < reached) mine.n += fa.coef[g.block_offset(m, s)];
    }
    jd::Counts all;
    const jd::Counts before = scan_counts(mine, scan_lds, &all);
    int pred = before.n;
    for (int m = m0; m < m1; ++m) {
      if (g.ri > 0 && m % g.ri == 0) pred = 0;
      for (int s = slot0; s < slot0 + slots; ++s) {
        if (m * g.bpm + s < reached) {
          int16_t* p = fa.coef + g.block_offset(m, s);
          pred += *p;
          *p = (int16_t)pred;
        }
      }
    }
  }
  if (tid == 0) {
    int st = status_lds;
    const long long done = (long long)total.c * g.ri * g.bpm + total.n;
    if (stop == ENT_THREADS && done < g.total_blocks()) st |= RTV_JPEG_STATUS_SHORT;
    status[t] = st;
    if (rounds) rounds[t] = round;
  }
}

// ------------------------------------------------------------------------------------------------------------------------- pixels
__global__ void __launch_bounds__(PX_THREADS) jpeg_pixels_kernel(const DecodeArgs a) {
  __shared__ int ws[32 * 64];                                    // 32 blocks between the two IDCT passes
  __shared__ int quant[3][64];
  __shared__ uint8_t luma[16][PX_MCUS * 16];
  __shared__ uint8_t chroma[2][24][(PX_MCUS + 2) * 8];
  const int tid = threadIdx.x, t = blockIdx.z, my = blockIdx.y, mx0 = blockIdx.x * PX_MCUS;
  const FrameArg& fa = a.f[t];
  const jd::Geom g = fa.g;
  if (my >= g.mcu_rows || mx0 >= g.mcu_cols) return;             // the grid is sized by the call's largest frame
  {
    const int* q = (const int*)(fa.frame + offsetof(rtv_jpeg_desc, quant));
    for (int i = tid; i < 192; i += PX_THREADS) quant[i >> 6][i & 63] = q[i];
  }
  const int nm = min(PX_MCUS, g.mcu_cols - mx0);                 // MCUs of this workgroup
  const int lw = nm * g.hs;                                      // luma blocks per block row
  const int nl = lw * g.vs;
  const bool sub = g.hs == 2;                                    // chroma subsampled (2x1 or 2x2): context blocks
  const int cb0 = sub ? mx0 - 1 : mx0, cbw = sub ? nm + 2 : nm;
  const int rb0 = g.vs == 2 ? my - 1 : my, cbh = g.vs == 2 ? 3 : 1;
  const int ncj = g.ncomp == 3 ? cbw * cbh : 0;
  const int jobs = nl + 2 * ncj;
  const int line = tid & 7;
  for (int j0 = 0; j0 < jobs; j0 += 32) {
    const int j = j0 + (tid >> 3);
    int comp = 0, grow = 0, gcol = 0, ly = 0, lx = 0;
    bool active = j < jobs;
    if (active) {
      if (j < nl) {
        const int br = j / lw, bc = j - br * lw;
        grow = my * g.vs + br, gcol = mx0 * g.hs + bc, ly = br * 8, lx = bc * 8;
      } else {
        const int k = j - nl;
        comp = 1 + k / ncj;
        const int kk = k - (comp - 1) * ncj, r = kk / cbw, c = kk - r * cbw;
        grow = rb0 + r, gcol = cb0 + c, ly = r * 8, lx = c * 8;
        active = grow >= 0 && grow < g.mcu_rows && gcol >= 0 && gcol < g.mcu_cols;
      }
    }
    __syncthreads();                                             // quant is loaded; the previous sweep is done with ws
    int in[8], out[8];
    int* w = ws + (tid >> 3) * 64;
    if (active) {                                                // columns
      const int16_t* blk = fa.coef + g.plane_offset(comp) + (grow * g.grid_w(comp) + gcol) * 64;
#pragma unroll
      for (int k = 0; k < 8; ++k) in[k] = (int)blk[k * 8 + line] * quant[comp][k * 8 + line];
      jd::idct8<true>(in, out);
#pragma unroll
      for (int k = 0; k < 8; ++k) w[k * 8 + line] = out[k];
    }
    __syncthreads();
    if (active) {                                                // rows
#pragma unroll
      for (int k = 0; k < 8; ++k) in[k] = w[line * 8 + k];
      jd::idct8<false>(in, out);
      uint8_t* dst = comp == 0 ? &luma[ly + line][lx] : &chroma[comp - 1][ly + line][lx];
#pragma unroll
      for (int k = 0; k < 8; ++k) dst[k] = (uint8_t)jd::range_limit(out[k]);
    }
  }
  __syncthreads();

  const int ph = g.vs * 8, pw = nm * g.hs * 8;                   // the tile in pixels
  const int y0 = my * ph, x0 = mx0 * g.hs * 8;
  const int ch = (g.H + g.vs - 1) / g.vs, cw = (g.W + g.hs - 1) / g.hs;   // the chroma planes' true size: edges replicate from there
  // chroma sample of component c at plane coordinates (cy, cx), clamped to the plane
  auto C = [&](int c, int cy, int cx) -> int {
    cy = min(max(cy, 0), ch - 1), cx = min(max(cx, 0), cw - 1);
    return chroma[c][cy - rb0 * 8][cx - cb0 * 8];
  };
  for (int i = tid; i < ph * pw; i += PX_THREADS) {
    const int py = i / pw, px = i - py * pw;
    const int Y = y0 + py, X = x0 + px;
    if (Y >= g.H || X >= g.W) continue;
    const int yv = luma[py][px];
    uint8_t* o = fa.out + ((size_t)Y * g.W + X) * 3;
    if (g.ncomp == 1) {
      o[0] = o[1] = o[2] = (uint8_t)yv;
      continue;
    }
    int cc[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      if (!sub) {
        cc[c] = C(c, Y, X);
      } else if (g.vs == 1) {                                    // h2v1 fancy: 3/4 nearer, 1/4 further
        const int cx = X >> 1, self = C(c, Y, cx);
        cc[c] = (X & 1) ? (3 * self + C(c, Y, cx + 1) + 2) >> 2 : (3 * self + C(c, Y, cx - 1) + 1) >> 2;
      } else {                                                   // h2v2 fancy: the same filter in both directions
        const int cx = X >> 1, cy = Y >> 1, ny = (Y & 1) ? cy + 1 : cy - 1;
        const int self = 3 * C(c, cy, cx) + C(c, ny, cx);
        if (X & 1) cc[c] = (3 * self + 3 * C(c, cy, cx + 1) + C(c, ny, cx + 1) + 7) >> 4;
        else cc[c] = (3 * self + 3 * C(c, cy, cx - 1) + C(c, ny, cx - 1) + 8) >> 4;
      }
    }
    uint8_t rgb[3];
    jd::ycc_to_rgb(yv, cc[0], cc[1], rgb);
    o[0] = rgb[0], o[1] = rgb[1], o[2] = rgb[2];
  }
}

// --------------------------------------------------------------------------------------------------------------------------- host
int fail(const char* fn, const char* why) {
  char msg[224];
  snprintf(msg, sizeof(msg), "%s: %s", fn, why);
  return set_error(-1, msg);
}

size_t frame_coef_bytes(const jd::Geom& g) { return ((size_t)g.coef_elems() * sizeof(int16_t) + 255) & ~(size_t)255; }

// validates everything but the pointers into the frames; fills args (coef pointers relative to arena) and the arena need
const char* plan(const rtv_jpeg_desc* descs, int T, int subseq_bits, DecodeArgs* args, size_t* need) {
  if (!descs) return "null argument";
  if (T < 1 || T > RTV_FRAMES_MAX) return "T must be in 1..RTV_FRAMES_MAX (16) frames per call";
  if (subseq_bits < 0 || (subseq_bits && (subseq_bits < 32 || subseq_bits % 32))) return "subseq_bits must be 0 or a multiple of 32, at least 32";
  size_t at = 0;
  for (int t = 0; t < T; ++t) {
    FrameArg& f = args->f[t];
    if (const char* why = jd::geom_from_desc(descs[t], &f.g)) return why;
    jd::Tables sel;
    sel.set(descs[t].comp_dc, descs[t].comp_ac);
    f.select = sel.select;
    f.coef = (int16_t*)at;
    at += frame_coef_bytes(f.g);
  }
  *need = at;
  return nullptr;
}

int launch_entropy(const char* fn, const DecodeArgs& args, int T, int subseq_bits, void* status, void* rounds, hipStream_t s) {
  double bytes = 0;
  for (int t = 0; t < T; ++t) bytes += (double)args.f[t].g.scan_bytes + 2.0 * args.f[t].g.coef_elems();
  ProfScope prof(PROF_MISC, s, bytes);
  hipLaunchKernelGGL(jpeg_entropy_decode_kernel, dim3(T), dim3(ENT_THREADS), 0, s, args, subseq_bits, (int*)status, (int*)rounds);
  return check_launch(fn);
}

int prepare(const char* fn, const rtv_jpeg_desc* descs, const void* const* frames, int T, int subseq_bits, void* arena, size_t arena_bytes,
            const void* status, DecodeArgs* args) {
  size_t need = 0;
  if (!frames || !arena || !status) return fail(fn, "null argument");
  if (const char* why = plan(descs, T, subseq_bits, args, &need)) return fail(fn, why);
  if (arena_bytes < need) return fail(fn, "arena smaller than rtv_jpeg_decode_arena_bytes(descs, T)");
  if ((uintptr_t)arena & 15) return fail(fn, "arena must be 16-byte aligned");
  for (int t = 0; t < T; ++t) {
    if (!frames[t]) return fail(fn, "null frame pointer");
    if ((uintptr_t)frames[t] & 15) return fail(fn, "a frame (descriptor plus file) must be 16-byte aligned");
    args->f[t].frame = (const uint8_t*)frames[t];
    args->f[t].coef = (int16_t*)((char*)arena + (size_t)args->f[t].coef);
    args->f[t].out = nullptr;
  }
  return 0;
}

}  // namespace
}  // namespace rtv

using namespace rtv;

extern "C" {

int rtv_jpeg_parse(const void* file, size_t file_bytes, rtv_jpeg_desc* desc) {
  if (!file || !desc) return fail("jpeg_parse", "null argument");
  if (const char* why = jd::parse((const uint8_t*)file, file_bytes, desc)) return fail("jpeg_parse", why);
  return 0;
}

size_t rtv_jpeg_decode_arena_bytes(const rtv_jpeg_desc* descs, int T) {
  DecodeArgs args;
  size_t need = 0;
  return plan(descs, T, 0, &args, &need) ? 0 : need;
}

int rtv_jpeg_decode(const rtv_jpeg_desc* descs, const void* const* frames, void* const* rgb8, int T, int subseq_bits, void* arena,
                    size_t arena_bytes, void* status, void* rounds, rtv_stream_t stream) {
  if (T == 0) return 0;
  DecodeArgs args = {};
  if (!rgb8) return fail("jpeg_decode", "null argument");
  if (int e = prepare("jpeg_decode", descs, frames, T, subseq_bits, arena, arena_bytes, status, &args)) return e;
  int rows = 0, cols = 0;
  double px = 0;
  for (int t = 0; t < T; ++t) {
    if (!rgb8[t]) return fail("jpeg_decode", "null output pointer");
    args.f[t].out = (uint8_t*)rgb8[t];
    rows = args.f[t].g.mcu_rows > rows ? args.f[t].g.mcu_rows : rows;
    cols = args.f[t].g.mcu_cols > cols ? args.f[t].g.mcu_cols : cols;
    px += (double)args.f[t].g.H * args.f[t].g.W;
  }
  hipStream_t s = (hipStream_t)stream;
  if (int e = launch_entropy("jpeg_decode (entropy)", args, T, subseq_bits, status, rounds, s)) return e;
  ProfScope prof(PROF_MISC, s, px * 6.0);
  hipLaunchKernelGGL(jpeg_pixels_kernel, dim3((cols + PX_MCUS - 1) / PX_MCUS, rows, T), dim3(PX_THREADS), 0, s, args);
  return check_launch("jpeg_decode (pixels)");
}

int rtv_jpeg_decode_coefficients(const rtv_jpeg_desc* desc, const void* frame, int subseq_bits, void* arena, size_t arena_bytes,
                                 void* coefficients, void* status, void* rounds, rtv_stream_t stream) {
  DecodeArgs args = {};
  if (!coefficients) return fail("jpeg_decode_coefficients", "null argument");
  const void* frames[1] = {frame};
  if (int e = prepare("jpeg_decode_coefficients", desc, frame ? frames : nullptr, 1, subseq_bits, arena, arena_bytes, status, &args)) return e;
  hipStream_t s = (hipStream_t)stream;
  if (int e = launch_entropy("jpeg_decode_coefficients", args, 1, subseq_bits, status, rounds, s)) return e;
  if (hipMemcpyAsync(coefficients, arena, (size_t)args.f[0].g.coef_elems() * sizeof(int16_t), hipMemcpyDeviceToDevice, s) != hipSuccess)
    return fail("jpeg_decode_coefficients", "copying the coefficients failed");
  return 0;
}

}  // extern "C"
