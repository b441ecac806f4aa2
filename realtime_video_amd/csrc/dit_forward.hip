// DiT forward orchestrator: CausalWanModel._forward_inference
// (wan/modules/causal_model.py:825-954; block body :440-492; head :495-523; unpatchify :1126-1149).
// Pure launch sequencing over the kernels of this library on ONE stream: no allocation, no sync, so
// every entry is hipGraph-capturable.  13 launches per DiT layer.
//
// Token-axis (context-parallel) sharding: a rank owns token rows [row_begin, row_begin + row_count) of the
// M = F*gh*gw tokens.  Every per-token op runs on the local rows only; the single exchange per layer is the
// all-gather of the new K/V rows into the replicated KV cache, done by the host (RCCL via torch.distributed)
// between rtv_dit_layer_qkv and rtv_dit_layer_rest.  rtv_dit_forward = the unsharded composition.
//
// Head-parallel exchange (the *_hp phases; the reference's usp_attn_forward, xdit_context_parallel.py:149-190, does the
// same through xFuserLongContextAttention): tokens stay sharded for every per-token op, but around self-attention the
// shard flips to heads - each rank attends ALL M query rows for its H/world heads over a KV cache that holds only those
// heads.  Two all-to-alls per layer (q|k|v out, attention output back) move 4*(M/world)*d*(world-1)/world elements per
// rank instead of the all-gather's 2*M*d*(world-1)/world: world/2 times less xGMI traffic.
#include <atomic>
#include <string>

#include "../../include/rtv_hip_attn_fp8.h"
#include "../../include/rtv_hip_attn_fp8_center.h"
#include "../../include/rtv_hip_attn_fp8_only_center.h"
#include "../../include/rtv_hip_attn_fp8_cp.h"
#include "../../include/rtv_hip_attn_fp8_only.h"
#include "../../include/rtv_hip_attn_fp8_only_cp.h"
#include "../../include/rtv_hip_mxfp4.h"
#include "../../include/rtv_hip_mxfp6.h"
#include "../../include/rtv_hip_mx_rotate.h"
#include "rtv_common.h"
#include "rtv_internal.h"

namespace rtv {

__global__ void silu_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = f32_to_bf16(silu(bf16_to_f32(x[i])));
}

// Folded cross-attention weight of one layer (rtv_cross_fold_weight): vo[n, h*kh + t] = sum_d' co_w[n, h*128 + d'] * v[t, h*128 + d'].
// Once per prompt, 0.03 % of a block's multiply-adds: plain fp32 FMAs.  Workgroup = 64 rows n of one head; lane = key t (so the
// 2-byte stores of a wave are one contiguous run), wave = 16 of the 64 rows.  LDS rows are 130 elements long: the per-lane reads
// of V (65 words apart) touch 64 different banks, the reads of co_w are broadcasts.
constexpr int FOLD_ROWS = 64, FOLD_LD = 130;
__global__ __launch_bounds__(256) void cross_fold_weight_kernel(const bf16_t* __restrict__ w, int64_t ldw, const bf16_t* __restrict__ v,
                                                               int64_t ldv, bf16_t* __restrict__ vo, int64_t ldvo, int H, int rows, int kh,
                                                               int k_fold) {
  __shared__ __attribute__((aligned(16))) bf16_t sW[FOLD_ROWS * FOLD_LD];
  __shared__ __attribute__((aligned(16))) bf16_t sV[128 * FOLD_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * FOLD_ROWS, h = blockIdx.y;
  for (int id = tid; id < FOLD_ROWS * 64; id += 256) {      // 2 elements per step (the padded rows are only 4-byte aligned)
    const int r = id >> 6, c = (id & 63) * 2;
    *(uint32_t*)(sW + r * FOLD_LD + c) = *(const uint32_t*)(w + (int64_t)(n0 + r) * ldw + h * 128 + c);
  }
  for (int id = tid; id < rows * 64; id += 256) {
    const int r = id >> 6, c = (id & 63) * 2;
    *(uint32_t*)(sV + r * FOLD_LD + c) = *(const uint32_t*)(v + (int64_t)r * ldv + h * 128 + c);
  }
  __syncthreads();
  for (int ts = 0; ts < kh; ts += 64) {
    const int t = ts + lane;
    float acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    if (t < rows) {
      const bf16_t* vr = sV + t * FOLD_LD;
      const bf16_t* wr = sW + wave * 16 * FOLD_LD;
      for (int dd = 0; dd < 128; dd += 2) {
        const uint32_t v2 = *(const uint32_t*)(vr + dd);
        const float v0 = __uint_as_float(v2 << 16), v1 = __uint_as_float(v2 & 0xffff0000u);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const uint32_t w2 = *(const uint32_t*)(wr + i * FOLD_LD + dd);
          acc[i] = fmaf(__uint_as_float(w2 << 16), v0, acc[i]);
          acc[i] = fmaf(__uint_as_float(w2 & 0xffff0000u), v1, acc[i]);
        }
      }
    }
    if (t < kh) {   // keys t >= rows of the head's kh columns: zeros
#pragma unroll
      for (int i = 0; i < 16; ++i) vo[(int64_t)(n0 + wave * 16 + i) * ldvo + h * kh + t] = f32_to_bf16(acc[i]);
    }
  }
  if (h == H - 1) {   // the tail behind the last head's columns
    const int tail0 = H * kh;
    for (int t = tail0 + lane; t < k_fold; t += 64)
#pragma unroll
      for (int i = 0; i < 16; ++i) vo[(int64_t)(n0 + wave * 16 + i) * ldvo + t] = 0;
  }
}

struct Workspace {
  char* base;
  size_t off, cap;
  bool ok;
  void* take(size_t bytes) {
    size_t a = (off + 255) & ~(size_t)255;
    if (base && a + bytes > cap) ok = false;
    off = a + bytes;
    return base ? base + a : nullptr;
  }
};

struct DitBuffers {
  uint16_t *x, *xn, *qkv, *q, *ao, *h, *prow, *hrow;
  uint16_t *sinus, *te1, *e, *se, *e0, *emod, *ehead, *ctx1, *ctx, *ktmp;
  uint8_t* q8;      // fp8 path: the quantised activation of the linear being computed (use_fp8 == 3, MXFP4: its e2m1 codes in the
                    // first rows * K / 2 bytes and its block scales behind them - 17 / 32 of the fp8 size; use_fp8 == 4, MXFP6: e2m3
                    // codes in the first rows * 3 K / 4 bytes, block scales behind them - 25 / 32; 5 / 6, the rotated modes: as 3 / 4)
  float* frow;      // fp8 path with per-row scales (use_fp8 == 2, and 7 for its Linears in mode 2): the row scales of the activation in q8
  float* fscale;    // fp8 path: its per-tensor scale (device), followed by the 4-byte absmax scratch
  float* attn_part; // KV-split self-attention of a sharded call: fp32 partial outputs + (m, l) of splits x heads x rows <= H x M
  size_t attn_part_bytes;
};

// Buffers are sized for the full token count so that one workspace serves sharded and unsharded calls.
static size_t carve(const rtv_dit_config* c, int F, int gh, int gw, char* base, size_t cap, DitBuffers* b,
                    bool* ok) {
  Workspace ws{base, 0, cap, true};
  const size_t M = (size_t)F * gh * gw, d = c->dim, e = 2;
  DitBuffers t;
  t.x = (uint16_t*)ws.take(M * d * e);
  t.xn = (uint16_t*)ws.take(M * d * e);
  t.qkv = (uint16_t*)ws.take(M * 3 * d * e);
  t.q = (uint16_t*)ws.take(M * d * e);
  t.ao = (uint16_t*)ws.take(M * d * e);
  t.h = (uint16_t*)ws.take(M * (size_t)c->ffn_dim * e);
  t.prow = (uint16_t*)ws.take(M * (size_t)c->in_dim * 4 * e);
  t.hrow = (uint16_t*)ws.take(M * (size_t)c->out_dim * 4 * e);
  t.sinus = (uint16_t*)ws.take((size_t)F * c->freq_dim * e);
  t.te1 = (uint16_t*)ws.take((size_t)F * d * e);
  t.e = (uint16_t*)ws.take((size_t)F * d * e);
  t.se = (uint16_t*)ws.take((size_t)F * d * e);
  t.e0 = (uint16_t*)ws.take((size_t)F * 6 * d * e);
  t.emod = (uint16_t*)ws.take((size_t)c->num_layers * F * 6 * d * e);
  t.ehead = (uint16_t*)ws.take((size_t)F * 2 * d * e);
  t.ctx1 = (uint16_t*)ws.take((size_t)c->text_len * d * e);
  t.ctx = (uint16_t*)ws.take((size_t)c->text_len * d * e);
  t.ktmp = (uint16_t*)ws.take((size_t)c->text_len * d * e);
  {
    size_t rows = M > (size_t)c->text_len ? M : (size_t)c->text_len, k = d;
    if ((size_t)c->ffn_dim > k) k = c->ffn_dim;
    if ((size_t)c->text_dim > k) k = c->text_dim;
    if ((size_t)c->freq_dim > k) k = c->freq_dim;
    t.q8 = (uint8_t*)ws.take(c->use_fp8 ? rows * k : 0);
    // (an empty take moves nothing: modes 0 / 1 keep their layout; 7, mixed: the union - q8 at the fp8 size, which covers both MX
    // layouts, the row scales, and the per-tensor slots below)
    t.frow = (float*)ws.take(c->use_fp8 == 2 || c->use_fp8 == 7 ? rows * sizeof(float) : 0);
    t.fscale = (float*)ws.take(256);
  }
  // KV-split self-attention of sharded calls, only when the configuration asks for it (97 MB per workspace at 14B
  // that an unsharded forward never touches).  A sharded call attends rows x heads <= M x H / world; with kv_splits <= world the
  // partials of all splits fit M x H rows.
  t.attn_part_bytes = c->max_attn_kv_splits > 1 ? M * (size_t)c->num_heads * (128 + 2) * sizeof(float) : 0;
  t.attn_part = (float*)ws.take(t.attn_part_bytes);
  if (b) *b = t;
  if (ok) *ok = ws.ok;
  return ws.off;
}

struct Ctx {
  const rtv_dit_config* cfg;
  const rtv_dit_weights* w;
  const rtv_dit_step* st;
  DitBuffers b;
  rtv_stream_t stream;
  int d, H, L, ffn, hd, F, gh, gw, fs, M, r0, rc, tc;
  const rtv_attn_fp8_shadow* fp8;   // rtv_dit_forward_attn_fp8 and the sharded phases of rtv_hip_attn_fp8_cp.h: self-attention on the
                                    // e4m3 shadows; null in every other entry point
  void* const* centers;             // rtv_dit_forward_attn_fp8_centered: per-layer K centres of the shadows; null in every other one
  bool fp8_only;                    // rtv_dit_forward_attn_fp8_only: the shadows ARE the cache - st->kv_k / kv_v / kv_row_stride are not read
  void* kv8;                        // the phases of rtv_hip_attn_fp8_only_cp.h: the staging buffer the K | V phase writes its codes into
  int kv8_world;                    // (with fp8_only; the cache itself is written by the commit behind the exchange); null otherwise
  const uint8_t* modes;  // use_fp8 == 7: the mode of each Linear (linear_modes, checked by make_ctx); null otherwise
  int fold_kh, fold_k;   // cross-attention V folded into the output projection: columns per head / in all; 0 = the unfolded path
                         // (then st->ca_v[L + l] is layer l's folded weight, rtv_dit_step.ca_vo_ld)
};

// use_fp8 == 7: the modes of the Linears, a host array of 6 + 8 L bytes whose address is the entry behind the 6 + 8 L scale entries
// of rtv_dit_weights.fp8_row_scales (the struct has no field for it: its layout is pinned).  Null when the table or the entry is.
static const uint8_t* linear_modes(const rtv_dit_config* cfg, const rtv_dit_weights* w) {
  return w->fp8_row_scales ? (const uint8_t*)w->fp8_row_scales[6 + 8 * (cfg->num_layers > 0 ? cfg->num_layers : 0)] : nullptr;
}

// use_fp8 == 7 (one mode per Linear): everything a Linear of that mode would ask for later is asked for here, in front of the first
// launch.  The order of the table is that of fp8_scales; K = the Linear's input width.
static int check_linear_modes(const rtv_dit_config* cfg, const rtv_dit_weights* w, const uint8_t* modes) {
  if (!modes) return set_error(-1, "dit: use_fp8 == 7 needs linear_modes (the last entry of rtv_dit_weights.fp8_row_scales)");
  static const char* const top[] = {"text0", "text2", "time0", "time2", "tproj", "head"};
  static const char* const per_layer[] = {"qkv", "o", "cq", "ck", "cv", "co", "ffn0", "ffn2"};
  const int n = 6 + 8 * cfg->num_layers;
  for (int i = 0; i < n; ++i) {
    const int mode = modes[i];
    const int K = i == 0 ? cfg->text_dim : i == 2 ? cfg->freq_dim : (i >= 6 && (i - 6) % 8 == 7) ? cfg->ffn_dim : cfg->dim;
    const int mult = mode == 3 || mode == 5 ? 256 : mode == 4 || mode == 6 ? 128 : 1;
    const char* what = mode > 6                                                        ? " is not a mode (0 to 6)"
                       : mode == 1 && !w->fp8_scales                                   ? " needs rtv_dit_weights.fp8_scales"
                       : mode >= 2 && (!w->fp8_row_scales || !w->fp8_row_scales[i])    ? " needs its rtv_dit_weights.fp8_row_scales entry"
                       : K % mult                                                      ? (mult == 256 ? " needs an input width that is a multiple of 256"
                                                                                                      : " needs an input width that is a multiple of 128")
                                                                                       : nullptr;
    if (what) {   // (the name is put together for the message alone: this loop runs in front of every forward)
      const std::string name = i < 6 ? std::string(top[i]) : "L" + std::to_string((i - 6) / 8) + "." + per_layer[(i - 6) % 8];
      return set_error(-1, ("dit: linear_modes: " + name + ": mode " + std::to_string(mode) + what).c_str());
    }
  }
  return 0;
}

static int make_ctx(const rtv_dit_config* cfg, const rtv_dit_weights* w, const rtv_dit_step* st, void* workspace,
                    size_t workspace_bytes, rtv_stream_t stream, Ctx* c) {
  if (!cfg || !w || !st || !workspace) return set_error(-1, "dit: null argument");
  c->cfg = cfg;
  c->w = w;
  c->st = st;
  c->fp8 = nullptr;
  c->centers = nullptr;
  c->fp8_only = false;
  c->kv8 = nullptr;
  c->kv8_world = 0;
  c->stream = stream;
  c->d = cfg->dim;
  c->H = cfg->num_heads;
  c->L = cfg->num_layers;
  c->ffn = cfg->ffn_dim;
  if (c->H <= 0 || c->d % c->H || c->d / c->H != 128) return set_error(-1, "dit: head_dim must be 128");
  c->modes = nullptr;
  if (cfg->use_fp8 == 7) {
    c->modes = linear_modes(cfg, w);
    const int s = check_linear_modes(cfg, w, c->modes);
    if (s) return s;
  }
  c->hd = 128;
  c->F = st->F;
  c->gh = st->gh;
  c->gw = st->gw;
  c->fs = st->gh * st->gw;
  c->M = st->F * c->fs;
  if (c->M <= 0) return set_error(-1, "dit: empty token grid");
  c->r0 = st->row_begin;
  c->rc = st->row_count > 0 ? st->row_count : c->M - st->row_begin;
  if (c->r0 < 0 || c->rc <= 0 || c->r0 + c->rc > c->M) return set_error(-1, "dit: local row range outside the token grid");
  if (st->kv_lo < 0 || st->kv_hi <= st->kv_lo) return set_error(-1, "dit: empty attention window");
  if (st->cache_row0 < 0 || st->cache_row0 + c->M > st->kv_hi)
    return set_error(-1, "dit: the rows written by this call must lie inside the attention window");
  if (st->ring_size < 0 || st->ring_lo < 0 || st->ring_shift < 0 || (st->ring_size > 0 && st->ring_shift >= st->ring_size) ||
      (st->ring_size > 0 && st->kv_hi > st->ring_lo + st->ring_size))
    return set_error(-1, "dit: bad ring window (0 <= ring_shift < ring_size, kv_hi <= ring_lo + ring_size)");
  if (st->ring_size > 0 && st->ring_shift > 0 && st->causal_block > 0)
    return set_error(-1, "dit: the block-causal recompute pass writes an unrotated cache (ring_shift must be 0)");
  if (((uintptr_t)workspace) & 255) return set_error(-1, "dit: workspace must be 256-byte aligned");
  bool ok = true;
  carve(cfg, c->F, c->gh, c->gw, (char*)workspace, workspace_bytes, &c->b, &ok);
  if (!ok) return set_error(-1, "dit: workspace too small (see rtv_dit_workspace_bytes)");
  c->tc = st->gemm_tile_cfg;
  // One decision for every entry point (whole forward, phase API, every shard): a function of the configuration and the step alone.
  c->fold_kh = c->fold_k = 0;
  if (st->ca_vo_ld > 0 && st->ca_v && !cfg->use_fp8 && st->text_rows > 0 && st->text_rows + 1 < cfg->text_len) {
    int kh = 0, kf = 0;
    if (rtv_cross_fold_dims(c->H, st->text_rows, &kh, &kf) && kf <= c->d) {
      if (st->ca_vo_ld < kf || (st->ca_vo_ld & 7)) return set_error(-1, "dit: ca_vo_ld must be a multiple of 8 and >= k_fold (rtv_cross_fold_dims)");
      c->fold_kh = kh;
      c->fold_k = kf;
    }
  }
  return 0;
}

}  // namespace rtv

using namespace rtv;

#define RTV_TRY(expr)        \
  do {                       \
    int _s = (expr);         \
    if (_s != 0) return _s;  \
  } while (0)

extern "C" int rtv_silu(const void* x, void* out, int64_t n, rtv_stream_t stream) {
  if (n <= 0) return 0;
  int blocks = (int)((n + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(silu_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x,
                     (bf16_t*)out, n);
  return check_launch("silu");
}

extern "C" int rtv_cross_fold_dims(int num_heads, int text_rows, int* kh, int* k_fold) {
  const int khv = text_rows >= 0 ? (text_rows + 1 + 7) & ~7 : 0;
  const int64_t kf = ((int64_t)num_heads * khv + 63) & ~(int64_t)63;
  if (kh) *kh = khv;
  if (k_fold) *k_fold = kf > 0x7fffffff ? 0 : (int)kf;
  return num_heads > 0 && text_rows > 0 && khv <= RTV_CROSS_FOLD_KH_MAX && kf <= 0x7fffffff;
}

extern "C" int rtv_cross_fold_weight(const void* co_w, int64_t ldw, const void* v, int64_t ldv, void* vo, int64_t ldvo, int num_heads,
                                     int rows, int kh, int k_fold, rtv_stream_t stream) {
  if (!co_w || !v || !vo) return set_error(-1, "cross_fold_weight: null argument");
  if (num_heads <= 0 || rows <= 0 || rows > kh || kh > 128 || (kh & 7)) return set_error(-1, "cross_fold_weight: need 0 < rows <= kh <= 128, kh % 8 == 0");
  const int64_t d = (int64_t)num_heads * 128;
  if ((int64_t)num_heads * kh > k_fold || k_fold > ldvo || ldw < d || ldv < d || ((ldw | ldv) & 1))
    return set_error(-1, "cross_fold_weight: need num_heads * kh <= k_fold <= ldvo and rows of num_heads * 128 elements");
  if (((uintptr_t)co_w | (uintptr_t)v) & 3) return set_error(-1, "cross_fold_weight: operands must be 4-byte aligned");
  ProfScope prof(PROF_MISC, (hipStream_t)stream, 2.0 * d * (double)num_heads * rows * 128);
  hipLaunchKernelGGL(cross_fold_weight_kernel, dim3((unsigned)(d / FOLD_ROWS), num_heads), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)co_w, ldw, (const bf16_t*)v, ldv, (bf16_t*)vo, ldvo, num_heads, rows, kh, k_fold);
  return check_launch("cross_fold_weight");
}

extern "C" size_t rtv_dit_workspace_bytes(const rtv_dit_config* cfg, int F, int gh, int gw) {
  if (!cfg || F <= 0 || gh <= 0 || gw <= 0) return 0;
  return carve(cfg, F, gh, gw, nullptr, 0, nullptr, nullptr) + 256;
}

// nn.Linear on `M` rows with optional fused epilogue; `row_off` = global index of row 0 for the per-frame gate.
// fp8 mode (cfg->use_fp8, release_server.py:179-182): every nn.Linear quantises its input per tensor (dynamic; use_fp8 == 2: per
// row, rtv_hip_fp8_rows.h) and multiplies e4m3 operands; `sidx` indexes the weight's per-tensor scale in rtv_dit_weights.fp8_scales (< 0: the op is
// not an nn.Linear - the Conv3d patch embedding - and stays bf16).
enum { S_TEXT0 = 0, S_TEXT2, S_TIME0, S_TIME2, S_TPROJ, S_HEAD, S_LAYER0 };
enum { S_QKV = 0, S_O, S_CQ, S_CK, S_CV, S_CO, S_FFN0, S_FFN2, S_PER_LAYER };
enum { FP8_TENSOR = 1, FP8_ROWS = 2, MODE_MXFP4 = 3, MODE_MXFP6 = 4, MODE_MXFP4_ROT = 5, MODE_MXFP6_ROT = 6, MODE_MIXED = 7 };   // the values of cfg->use_fp8 (0: bf16)
// How Linear `sidx` runs, 0 to 6: the one mode of the model, or under MODE_MIXED the Linear's own (make_ctx has checked the table).
static int mode_of(const Ctx& c, int sidx) {
  if (sidx < 0) return 0;
  return c.cfg->use_fp8 == MODE_MIXED ? c.modes[sidx] : c.cfg->use_fp8;
}
static bool is_fp8(const Ctx& c, int sidx) { return mode_of(c, sidx) != 0; }

// A block-scaled mode (rtv_hip_mxfp4.h, rtv_hip_mxfp6.h): q8 holds an activation's codes, code_bytes(K) per row, then its scales.
// The rotated modes (rtv_hip_mx_rotate.h) are the same rows with the rotated quantisers: the weights were rotated at the weight shift
// when they were quantised, the activations are at the activation shift here, and the GEMM is the unrotated mode's.
struct MxMode {
  int (*code_bytes)(int K);
  decltype(&rtv_quantize_mxfp4) quantize;
  decltype(&rtv_layernorm_modulate_mxfp4) layernorm_modulate;
  decltype(&rtv_gemm_mxfp4) gemm;
};
template <decltype(&rtv_quantize_mxfp4_rot) Q>
static int quantize_act_rot(const void* x, int64_t ld, int M, int d, void* codes, int64_t ld_codes, void* scales, int64_t ld_scales,
                            rtv_stream_t s) {
  return Q(x, ld, M, d, codes, ld_codes, scales, ld_scales, RTV_MX_ROT_ACT_SHIFT, s);
}
static const MxMode MX_MODES[] = {   // [mode - MODE_MXFP4]
    {[](int K) { return K / 2; }, rtv_quantize_mxfp4, rtv_layernorm_modulate_mxfp4, rtv_gemm_mxfp4},
    {[](int K) { return RTV_MXFP6_CODE_BYTES(K); }, rtv_quantize_mxfp6, rtv_layernorm_modulate_mxfp6, rtv_gemm_mxfp6},
    {[](int K) { return K / 2; }, quantize_act_rot<rtv_quantize_mxfp4_rot>, rtv_layernorm_modulate_mxfp4_rot, rtv_gemm_mxfp4},
    {[](int K) { return RTV_MXFP6_CODE_BYTES(K); }, quantize_act_rot<rtv_quantize_mxfp6_rot>, rtv_layernorm_modulate_mxfp6_rot,
     rtv_gemm_mxfp6},
};
static const MxMode* mx_mode(const Ctx& c, int sidx) {
  const int mode = mode_of(c, sidx);
  return mode >= MODE_MXFP4 && mode <= MODE_MXFP6_ROT ? &MX_MODES[mode - MODE_MXFP4] : nullptr;
}
static uint8_t* mx_scales(const Ctx& c, const MxMode& mx, int M, int K) { return c.b.q8 + (size_t)M * mx.code_bytes(K); }

// Quantise half of a Linear: its input `a` [M][K] becomes e4m3 codes in q8 and the mode's scales in fscale / frow.  Nothing to do in
// bf16, and nothing when a == nullptr: the input is in q8 / frow already (ln_input: the LayerNorm in front of this Linear quantised
// its own output).  The weight's scales are asked for here, in front of the first launch of the Linear.
static int quantize_input(Ctx& c, int sidx, const void* a, int M, int K, rtv_stream_t s) {
  if (!is_fp8(c, sidx)) return 0;
  const int mode = mode_of(c, sidx);
  if (const MxMode* mx = mx_mode(c, sidx)) {
    // per 32-element block: like the row scales, the decisions of a row need that row alone
    if (!c.w->fp8_row_scales || !c.w->fp8_row_scales[sidx])
      return set_error(-1, ("dit: use_fp8 == " + std::to_string(mode) + " needs rtv_dit_weights.fp8_row_scales").c_str());
    return a ? mx->quantize(a, K, M, K, c.b.q8, mx->code_bytes(K), mx_scales(c, *mx, M, K), K / 32, s) : 0;
  }
  if (mode == FP8_ROWS) {
    // per-row scales: the quantisation of a row needs that row alone, so a token shard takes the unsharded forward's decisions
    if (!c.w->fp8_row_scales || !c.w->fp8_row_scales[sidx]) return set_error(-1, "dit: use_fp8 == 2 needs rtv_dit_weights.fp8_row_scales");
    return a ? rtv_quantize_fp8_rows(a, K, M, K, c.b.q8, K, c.b.frow, s) : 0;
  }
  if (!c.w->fp8_scales) return set_error(-1, "dit: use_fp8 needs rtv_dit_weights.fp8_scales");
  // token-sharded calls quantise the rows this rank holds with their own scale - what a per-rank torchao linear does
  return rtv_quantize_fp8(a, K, M, K, c.b.q8, K, c.b.fscale, c.b.fscale + 1, s) ? -1 : 0;
}

// Project half: output columns [w_row0, w_row0 + N) of the Linear = that row range of its weight [..][K] and of its bias, into
// out [M][ldc], from `a` (bf16) or from what quantize_input left.  A per-tensor scale holds for the weight whichever rows a launch
// takes; of the row scales it takes the matching slice.
static int project(Ctx& c, int sidx, const void* a, int K, const void* w, int w_row0, const void* bias, void* out, int ldc, int M, int N,
                   int act, const void* gate, int gate_stride, int rpf, int row_off, const void* res, int cfg, rtv_stream_t s) {
  const bool fp8 = is_fp8(c, sidx);
  const MxMode* mx = mx_mode(c, sidx);
  // fp8 weights are bytes, MXFP4 nibbles, MXFP6 three bytes per four elements
  const void* wp = (const char*)w + (size_t)w_row0 * (mx ? mx->code_bytes(K) : K * (fp8 ? 1 : 2));
  const void* bp = bias ? (const uint16_t*)bias + w_row0 : nullptr;
  const int ldr = res ? ldc : 0;
  if (!fp8) return rtv_gemm(a, K, wp, K, out, ldc, M, N, K, bp, act, gate, gate_stride, rpf, row_off, res, ldr, RTV_DTYPE_BF16, cfg, s);
  if (mx)
    return mx->gemm(c.b.q8, mx->code_bytes(K), wp, mx->code_bytes(K), mx_scales(c, *mx, M, K),
                    (const uint8_t*)c.w->fp8_row_scales[sidx] + (size_t)w_row0 * (K / 32), out, ldc, M, N, K, bp, act, gate, gate_stride, rpf,
                    row_off, res, ldr, s);
  if (mode_of(c, sidx) == FP8_ROWS)
    return rtv_gemm_fp8_rows(c.b.q8, K, wp, K, c.b.frow, (const float*)c.w->fp8_row_scales[sidx] + w_row0, out, ldc, M, N, K, bp, act, gate,
                             gate_stride, rpf, row_off, res, ldr, s);
  return rtv_gemm_fp8(c.b.q8, K, wp, K, c.b.fscale, c.w->fp8_scales[sidx], out, ldc, M, N, K, bp, act, gate, gate_stride, rpf, row_off, res,
                      ldr, s);
}

static int linear(Ctx& c, int sidx, const void* a, int K, const void* w, const void* bias, void* out, int M, int N, int act,
                  const void* gate, int gate_stride, int rpf, int row_off, const void* res, int cfg, rtv_stream_t s) {
  RTV_TRY(quantize_input(c, sidx, a, M, K, s));
  return project(c, sidx, a, K, w, 0, bias, out, N, M, N, act, gate, gate_stride, rpf, row_off, res, cfg, s);
}

// LayerNorm of the local rows of b.x in front of a Linear: modulated by (shift, scale) per frame, or affine (weight, bias).
// The result goes to b.xn - or, with per-row fp8 scales, straight to e4m3 codes and row scales in q8 / frow: one kernel in place
// of LayerNorm + quantiser, same bits.  *a = what linear() takes as that Linear's input (null: already quantised).  `sidx` is the
// Linear that consumes the result (qkv, cq, ffn0): its mode chooses the form.
static int ln_input(Ctx& c, int sidx, const void* shift, const void* scale, int frame_stride, const void* weight, const void* bias, const void** a) {
  DitBuffers& b = c.b;
  const int rpf = scale ? c.fs : 0, r0 = scale ? c.r0 : 0;
  if (const MxMode* mx = mx_mode(c, sidx)) {
    *a = nullptr;
    return mx->layernorm_modulate(b.x, b.q8, mx->code_bytes(c.d), mx_scales(c, *mx, c.rc, c.d), c.d / 32, c.rc, c.d, c.cfg->eps, shift, scale,
                                  frame_stride, rpf, r0, weight, bias, c.stream);
  }
  if (mode_of(c, sidx) == FP8_ROWS) {
    *a = nullptr;
    return rtv_layernorm_modulate_fp8_rows(b.x, b.q8, c.d, b.frow, c.rc, c.d, c.cfg->eps, shift, scale, frame_stride, rpf, r0, weight, bias,
                                           c.stream);
  }
  *a = b.xn;
  return rtv_layernorm_modulate(b.x, b.xn, c.rc, c.d, c.cfg->eps, shift, scale, frame_stride, rpf, r0, weight, bias, c.stream);
}

// ---- embeddings, modulation tables, cross-attention K/V (causal_model.py:874-902)
static int dit_begin(Ctx& c) {
  const rtv_dit_config* cfg = c.cfg;
  const rtv_dit_weights* w = c.w;
  const rtv_dit_step* st = c.st;
  DitBuffers& b = c.b;
  const int d = c.d, F = c.F, L = c.L, tc = c.tc;
  rtv_stream_t stream = c.stream;
  const int pk = cfg->in_dim * 4;
  RTV_TRY(rtv_patchify(st->x, b.prow, cfg->in_dim, F, c.gh, c.gw, stream));
  RTV_TRY(linear(c, -1, b.prow + (size_t)c.r0 * pk, pk, w->patch_w, w->patch_b, b.x, c.rc, d, 0, nullptr, 0, 0, 0, nullptr, tc, stream));
  RTV_TRY(rtv_sinusoidal_embedding(st->t, b.sinus, F, cfg->freq_dim, stream));
  RTV_TRY(linear(c, S_TIME0, b.sinus, cfg->freq_dim, w->time0_w, w->time0_b, b.te1, F, d, RTV_ACT_SILU, nullptr, 0, 0, 0, nullptr, tc, stream));
  RTV_TRY(linear(c, S_TIME2, b.te1, d, w->time2_w, w->time2_b, b.e, F, d, 0, nullptr, 0, 0, 0, nullptr, tc, stream));
  RTV_TRY(rtv_silu(b.e, b.se, (int64_t)F * d, stream));
  RTV_TRY(linear(c, S_TPROJ, b.se, d, w->tproj_w, w->tproj_b, b.e0, F, 6 * d, 0, nullptr, 0, 0, 0, nullptr, tc, stream));
  RTV_TRY(rtv_modulation_table(w->modulation, b.e0, b.emod, L, F, 6, 6, d, stream));
  RTV_TRY(rtv_modulation_table(w->head_modulation, b.e, b.ehead, 1, F, 2, 1, d, stream));
  // text context -> cross-attention K/V caches, only while they are not initialised (model.py:186-192;
  // the text MLP output is consumed nowhere else, causal_model.py:897-902).  Replicated on every rank.
  if (st->compute_cross_kv) {
    if (!st->context) return set_error(-1, "dit: context required to initialise the cross-attention cache");
    const int T = cfg->text_len;
    RTV_TRY(linear(c, S_TEXT0, st->context, cfg->text_dim, w->text0_w, w->text0_b, b.ctx1, T, d, RTV_ACT_GELU_TANH, nullptr, 0, 0, 0, nullptr, tc, stream));
    RTV_TRY(linear(c, S_TEXT2, b.ctx1, d, w->text2_w, w->text2_b, b.ctx, T, d, 0, nullptr, 0, 0, 0, nullptr, tc, stream));
    for (int l = 0; l < L; ++l) {
      const rtv_dit_layer_weights& lw = w->layers[l];
      RTV_TRY(linear(c, S_LAYER0 + S_PER_LAYER * l + S_CK, b.ctx, d, lw.ck_w, lw.ck_b, b.ktmp, T, d, 0, nullptr, 0, 0, 0, nullptr, tc, stream));
      RTV_TRY(rtv_rmsnorm(b.ktmp, d, st->ca_k[l], d, T, d, cfg->eps, lw.cnorm_k_w, stream));
      RTV_TRY(linear(c, S_LAYER0 + S_PER_LAYER * l + S_CV, b.ctx, d, lw.cv_w, lw.cv_b, st->ca_v[l], T, d, 0, nullptr, 0, 0, 0, nullptr, tc, stream));
      if (c.fold_k)   // the folded weight lives and dies with the caches: refreshed exactly when they are (new prompt, LoRA change)
        RTV_TRY(rtv_cross_fold_weight(lw.co_w, d, st->ca_v[l], d, st->ca_v[c.L + l], st->ca_vo_ld, c.H, st->text_rows + 1, c.fold_kh, c.fold_k,
                                      stream));
    }
  }
  return 0;
}

static int hp_check(Ctx& c, int world);
static int quantize_written_rows(Ctx& c, int l);
static int write_fp8_only_rows(Ctx& c, int l, bool q);
static int stage_fp8_only_rows(Ctx& c, int l, bool q, bool kv);

// ---- layer, part 1: LN+modulate -> QKV -> RMSNorm(q,k)+RoPE -> local K/V rows into the cache (or the exchange buffers).
// `parts` selects what this call does, so that the host can put a collective between the two projections and let it run
// under the other one (RTV_PROJ_*): LN (the shared input of both), Q (columns [0, d) of the fused QKV weight), KV (columns
// [d, 3d)).  q_send / kv_send non-null = head-parallel exchange buffers (see below), null = local q + cache rows.
static std::atomic<void*> g_capture_q{nullptr}, g_capture_o{nullptr};   // rtv_dit_lab_capture_self_attn (test hook, rtv_hip_attn_fp8.h)
static std::atomic<int> g_direct_v{1};   // rtv_dit_set_direct_v(0): the V cache rows are copied by the RoPE / cache kernel (r04 form; A/B, tests)
static int dit_layer_proj(Ctx& c, int l, int parts, int world, void* q_send, void* kv_send) {
  const rtv_dit_layer_weights& lw = c.w->layers[l];
  const rtv_dit_step* st = c.st;
  DitBuffers& b = c.b;
  const int d = c.d;
  if (!(parts & (RTV_PROJ_LN | RTV_PROJ_Q | RTV_PROJ_KV))) return set_error(-1, "dit: empty projection phase");
  const uint16_t* em = b.emod + (size_t)l * c.F * 6 * d;  // [F][6][d]: shift_sa, scale_sa, gate_sa, shift_ffn, scale_ffn, gate_ffn
  // (per-row fp8 scales: the LN phase leaves codes and row scales in q8 / frow, and they stay there for the Q and KV phases of
  // this layer, as b.xn does in the other modes - no other Linear runs between the projection phases of a layer)
  if (parts & RTV_PROJ_LN) {
    const void* ln_out;   // b.xn or q8 / frow: the projections below read them by name
    RTV_TRY(ln_input(c, S_LAYER0 + S_PER_LAYER * l + S_QKV, em + 0 * d, em + 1 * d, 6 * d, nullptr, nullptr, &ln_out));
  }
  const bool q = parts & RTV_PROJ_Q, kv = parts & RTV_PROJ_KV;
  if (!q && !kv) return 0;
  // the fused weight is [3d, d] row-major: a column range of the output is a row range of the weight
  const int n0 = q ? 0 : d, nn = (q ? d : 0) + (kv ? 2 * d : 0);
  bool v_in_place = false;
  {
    // r05: when this call's cache rows are ONE physical row range (always, unless a ring write wraps), the V third of the projection
    // is a GEMM of its own whose output matrix IS those rows of the V cache; the RoPE / cache kernel then moves a third less
    // (rope_parts | 4).  (One launch with a second output matrix was built first: three more kernel arguments, or one more epilogue
    // instantiation, cost the ping-pong kernel 3-4 % on the ffn-in shape - more than the copy.)
    void* v_dst = nullptr;
    if (kv && !kv_send && !c.fp8_only && g_direct_v.load(std::memory_order_relaxed) && st->kv_v[l] && !(st->kv_row_stride & 7)) {
      int r0 = st->cache_row0 + c.r0;
      const int S = st->ring_lo, R = st->ring_size;
      bool one_range = true;
      if (R > 0 && r0 + c.rc > S) {
        if (r0 < S) one_range = false;                          // sink rows and ring rows in one call
        else {
          r0 = S + (r0 - S + st->ring_shift) % R;
          one_range = r0 + c.rc <= S + R;
        }
      }
      uint16_t* dst = (uint16_t*)st->kv_v[l] + (size_t)r0 * st->kv_row_stride;
      if (one_range && !((uintptr_t)dst & 15)) v_dst = dst;
    }
    // Everything the RoPE / cache launch behind the GEMMs would refuse is refused HERE, before a GEMM has written V rows into the
    // cache (a failing call used to leave the V rows overwritten and the K rows untouched).
    {
      const int rp = (q ? 1 : 0) | (kv ? 2 : 0) | (v_dst ? 4 : 0);
      if (q_send || kv_send) {
        RTV_TRY(hp_check(c, world));
        const int gc = d / world;
        if ((q && !q_send) || (kv && !kv_send)) return set_error(-1, "dit: exchange buffers required");
        RTV_TRY(qk_norm_rope_check(2 * gc, 0, c.rc, d, c.H, c.F, c.gh, c.gw, st->start_frame, c.r0, gc, (int64_t)c.rc * gc,
                                   (int64_t)c.rc * 2 * gc, 0, 0, 0, rp));
      } else {
        RTV_TRY(qk_norm_rope_check(c.fp8_only ? d : st->kv_row_stride, st->cache_row0, c.rc, d, c.H, c.F, c.gh, c.gw, st->start_frame, c.r0, 0, 0, 0,
                                   st->ring_lo, st->ring_size, st->ring_shift, rp));
      }
    }
    const int sidx = S_LAYER0 + S_PER_LAYER * l + S_QKV;
    const void* a = mode_of(c, sidx) >= FP8_ROWS ? nullptr : b.xn;   // what the LN phase left: b.xn, or codes and scales in q8 / frow (modes 2 to 6)
    RTV_TRY(quantize_input(c, sidx, a, c.rc, d, c.stream));
    auto proj = [&](int w_row0, int N, void* out, int ldc) {
      return project(c, sidx, a, d, lw.qkv_w, w_row0, lw.qkv_b, out, ldc, c.rc, N, 0, nullptr, 0, 0, 0, nullptr, c.tc, c.stream);
    };
    if (v_dst) {
      // two launches: columns [n0, 2d) into the projection buffer, the V third straight into the cache rows (Q | K at M = 4680 is 760
      // tiles = 2.97 rounds of the 256 CUs, V the o-projection's shape: +6 us on the fused launch's 563, against the 21 us the copy cost)
      if (2 * d > n0) RTV_TRY(proj(n0, 2 * d - n0, b.qkv + n0, 3 * d));
      RTV_TRY(proj(2 * d, d, v_dst, (int)st->kv_row_stride));
      v_in_place = true;
    } else {
      RTV_TRY(proj(n0, nn, b.qkv + n0, 3 * d));
    }
  }
  const int rope_parts = (q ? 1 : 0) | (kv ? 2 : 0) | (v_in_place ? 4 : 0);
  if (q_send || kv_send) {
    RTV_TRY(hp_check(c, world));
    const int gc = d / world;
    if ((q && !q_send) || (kv && !kv_send)) return set_error(-1, "dit: exchange buffers required");
    return qk_norm_rope_launch(b.qkv, q_send, kv_send, kv_send ? (void*)((uint16_t*)kv_send + gc) : nullptr, 2 * gc, 0, c.rc, d, c.H,
                               c.cfg->eps, lw.norm_q_w, lw.norm_k_w, c.w->rope_cs, c.F, c.gh, c.gw, st->start_frame, c.r0, gc,
                               (int64_t)c.rc * gc, (int64_t)c.rc * 2 * gc, 0, 0, 0, rope_parts, c.stream);
  }
  if (c.fp8_only && c.kv8) return stage_fp8_only_rows(c, l, q, kv);   // rtv_dit_layer_proj_attn_fp8_only: codes into the staging buffer
  if (c.fp8_only) return write_fp8_only_rows(c, l, q);   // (never with exchange buffers: the mode refuses sharded steps)
  RTV_TRY(qk_norm_rope_launch(b.qkv, b.q, st->kv_k[l], st->kv_v[l], st->kv_row_stride, st->cache_row0, c.rc, d, c.H, c.cfg->eps,
                              lw.norm_q_w, lw.norm_k_w, c.w->rope_cs, c.F, c.gh, c.gw, st->start_frame, c.r0, 0, 0, 0, st->ring_lo,
                              st->ring_size, st->ring_shift, rope_parts, c.stream));
  if (kv && c.fp8) return quantize_written_rows(c, l);   // K and V rows (direct V GEMM included) are in the cache here
  return 0;
}

// The physical cache rows of the logical rows [a, a + n) by the ring mapping of the write: sink rows as they are, ring rows rotated,
// at most one wrap.  -> the number of segments (first physical row, rows) in seg, in the order of the logical rows; -1: refused.
static int cut_written_rows(const rtv_dit_step* st, int a, int n, int seg[3][2]) {
  const int S = st->ring_lo, R = st->ring_size;
  int ns = 0;
  if (R <= 0) {
    seg[ns][0] = a, seg[ns++][1] = n;
  } else {
    if (a < S) {
      const int m = n < S - a ? n : S - a;
      seg[ns][0] = a, seg[ns++][1] = m;
      a += m, n -= m;
    }
    if (n > 0) {
      const int p0 = S + (a - S + st->ring_shift) % R;
      const int first = n < S + R - p0 ? n : S + R - p0;
      seg[ns][0] = p0, seg[ns++][1] = first;
      if (n - first > R) return set_error(-1, "dit: fp8 attention: a call writes more rows than the ring holds");
      if (n > first) seg[ns][0] = S, seg[ns++][1] = n - first;
    }
  }
  return ns;
}

// fp8 attention: the physical cache rows of the logical rows [a, a + n) of layer l go into the layer's e4m3 shadow, `heads` heads
// of them.
static int quantize_cache_rows(const rtv_dit_step* st, const rtv_attn_fp8_shadow* sh, void* const* centers, int l, int a, int n,
                               int heads, rtv_stream_t stream) {
  if (!sh->k8[l] || !sh->v8t[l]) return set_error(-1, "dit: fp8 attention: a layer has no shadow");
  int seg[3][2];
  const int ns = cut_written_rows(st, a, n, seg);
  if (ns < 0) return ns;
  void* amax = sh->amax ? sh->amax[l] : nullptr;
  for (int i = 0; i < ns; ++i) {
    if (centers)
      RTV_TRY(rtv_attn_quantize_kv_centered(st->kv_k[l], st->kv_v[l], st->kv_row_stride, seg[i][0], seg[i][1], heads, sh->k8[l],
                                            sh->v8t[l], sh->cache_rows, sh->k_scale, sh->v_scale, amax, (const float*)centers[l],
                                            stream));
    else
      RTV_TRY(rtv_attn_quantize_kv(st->kv_k[l], st->kv_v[l], st->kv_row_stride, seg[i][0], seg[i][1], heads, sh->k8[l], sh->v8t[l],
                                   sh->cache_rows, sh->k_scale, sh->v_scale, amax, stream));
  }
  return 0;
}

// ... the rows this call has just written
static int quantize_written_rows(Ctx& c, int l) {
  return quantize_cache_rows(c.st, c.fp8, c.centers, l, c.st->cache_row0 + c.r0, c.rc, c.H, c.stream);
}

// The e4m3-only cache (rtv_hip_attn_fp8_only.h): the block's q rows into b.q and its K rows into k8 in one launch, then its V rows
// from the V third of the projection buffer into v8t, one launch per physical segment.
static int write_fp8_only_rows(Ctx& c, int l, bool q) {
  const rtv_dit_layer_weights& lw = c.w->layers[l];
  const rtv_dit_step* st = c.st;
  const rtv_attn_fp8_shadow* sh = c.fp8;
  const int d = c.d;
  void* amax = sh->amax ? sh->amax[l] : nullptr;
  int seg[3][2];
  const int ns = cut_written_rows(st, st->cache_row0 + c.r0, c.rc, seg);
  if (ns < 0) return ns;
  if (c.centers)   // rtv_dit_forward_attn_fp8_only_centered: the K codes of k - centre
    RTV_TRY(rtv_qk_norm_rope_k8_centered(c.b.qkv, q ? c.b.q : nullptr, sh->k8[l], sh->cache_rows, sh->k_scale, amax, st->cache_row0, c.rc,
                                         d, c.H, c.cfg->eps, lw.norm_q_w, lw.norm_k_w, c.w->rope_cs, c.F, c.gh, c.gw, st->start_frame,
                                         c.r0, st->ring_lo, st->ring_size, st->ring_shift, (const float*)c.centers[l], c.stream));
  else
    RTV_TRY(rtv_qk_norm_rope_k8(c.b.qkv, q ? c.b.q : nullptr, sh->k8[l], sh->cache_rows, sh->k_scale, amax, st->cache_row0, c.rc, d, c.H,
                                c.cfg->eps, lw.norm_q_w, lw.norm_k_w, c.w->rope_cs, c.F, c.gh, c.gw, st->start_frame, c.r0, st->ring_lo,
                                st->ring_size, st->ring_shift, c.stream));
  const uint16_t* v_src = c.b.qkv + 2 * d;
  for (int i = 0; i < ns; ++i) {
    RTV_TRY(rtv_attn_quantize_v_rows(v_src, 3 * d, seg[i][1], c.H, sh->v8t[l], sh->cache_rows, seg[i][0], sh->v_scale, amax, c.stream));
    v_src += (size_t)seg[i][1] * 3 * d;
  }
  return 0;
}

// The e4m3-only cache under the row exchange (rtv_hip_attn_fp8_only_cp.h): the q rows into b.q as the bf16 path writes them, the
// codes of the local K and V rows into the rank's segment of the staging buffer.  The cache is written behind the exchange.
static int stage_fp8_only_rows(Ctx& c, int l, bool q, bool kv) {
  const rtv_dit_layer_weights& lw = c.w->layers[l];
  const rtv_dit_step* st = c.st;
  const rtv_attn_fp8_shadow* sh = c.fp8;
  const int d = c.d;
  if (q)
    RTV_TRY(qk_norm_rope_launch(c.b.qkv, c.b.q, nullptr, nullptr, d, st->cache_row0, c.rc, d, c.H, c.cfg->eps, lw.norm_q_w, lw.norm_k_w,
                                c.w->rope_cs, c.F, c.gh, c.gw, st->start_frame, c.r0, 0, 0, 0, st->ring_lo, st->ring_size,
                                st->ring_shift, 1, c.stream));
  if (kv)
    RTV_TRY(rtv_attn_fp8_stage_kv8(c.b.qkv, c.kv8, c.kv8_world, c.r0, c.rc, sh->k_scale, sh->v_scale, sh->amax ? sh->amax[l] : nullptr, d,
                                   c.H, c.cfg->eps, lw.norm_k_w, c.w->rope_cs, c.F, c.gh, c.gw, st->start_frame, c.stream));
  return 0;
}

static int dit_layer_qkv(Ctx& c, int l) { return dit_layer_proj(c, l, RTV_PROJ_LN | RTV_PROJ_Q | RTV_PROJ_KV, 0, nullptr, nullptr); }

static int dit_after_attn(Ctx& c, int l);

// Physical row ranges of the logical attention window [kv_lo, kv_hi) of a ring-indexed cache: at most two, because the
// sink rows [.., ring_lo) are adjacent to the ring's first physical row and the ring part wraps at most once.
struct KeyWindow {
  int row0, n0, row1, n1;
};
static KeyWindow key_window(const rtv_dit_step* st) {
  const int lo = st->kv_lo, hi = st->kv_hi, S = st->ring_lo, R = st->ring_size;
  if (R <= 0 || hi <= S) return KeyWindow{lo, hi - lo, 0, 0};
  const int rl = lo > S ? lo : S;                       // logical start of the ring part
  const int n = hi - rl;                                // ring rows in the window
  const int p0 = S + (rl - S + st->ring_shift) % R;     // its first physical row
  const int first = (p0 + n <= S + R) ? n : S + R - p0; // rows before the wrap
  const int sink = lo < S ? S - lo : 0;
  if (first == n) {                                     // no wrap: [lo, S) then [p0, p0 + n)
    if (sink == 0) return KeyWindow{p0, n, 0, 0};
    if (p0 == S) return KeyWindow{lo, sink + n, 0, 0};
    return KeyWindow{lo, sink, p0, n};
  }
  // wrapped: [p0, S + R) and [S, S + n - first); the sink rows are adjacent to the second piece
  return KeyWindow{sink ? lo : S, sink + n - first, p0, first};
}

// Self-attention of a sharded call: one launch, or the KV-split one when the step asks for it (an error when the workspace was
// not sized for it: never a silent unsplit run).
static int sharded_self_attn(Ctx& c, const void* q, const void* k, const void* v, void* o, int rows, int n0, int n1, int seg1_row,
                             int heads, int64_t q_rs, int64_t kv_rs, int64_t o_rs, int q_offset) {
  const rtv_dit_step* st = c.st;
  const float scale = 1.0f / sqrtf((float)c.hd);
  const int S = st->attn_kv_splits;
  const int qo = st->causal_block > 0 ? q_offset : 0;
  if (S > 1 && (S > c.cfg->max_attn_kv_splits || rtv_attn_split_workspace_bytes(1, rows, heads, S) > c.b.attn_part_bytes))
    return set_error(-1, "dit: attn_kv_splits exceeds rtv_dit_config.max_attn_kv_splits / the partials do not fit the workspace "
                         "(splits <= number of shards)");
  if (S > 1)
    return rtv_attn_fwd_split(q, k, v, o, 1, rows, n0, n1, seg1_row, heads, c.hd, 0, q_rs, 0, kv_rs, 0, kv_rs, 0, o_rs, scale,
                              st->causal_block, qo, S, c.b.attn_part, c.b.attn_part_bytes, RTV_DTYPE_BF16, c.stream);
  return rtv_attn_fwd_win(q, k, v, o, 1, rows, n0, n1, seg1_row, heads, c.hd, 0, q_rs, 0, kv_rs, 0, kv_rs, 0, o_rs, scale,
                          st->causal_block, qo, RTV_DTYPE_BF16, c.stream);
}

// The bounds check of sharded_self_attn for the fp8 split; the fp8 phases make it in front of their first launch as well.
static int check_fp8_split(const Ctx& c, int rows, int heads) {
  const int S = c.st->attn_kv_splits;
  if (S > 1 && (S > c.cfg->max_attn_kv_splits || rtv_attn_split_workspace_bytes(1, rows, heads, S) > c.b.attn_part_bytes))
    return set_error(-1, "dit: attn_kv_splits exceeds rtv_dit_config.max_attn_kv_splits / the partials do not fit the workspace "
                         "(splits <= number of shards)");
  return 0;
}

// Self-attention on the e4m3 shadow: one launch, or - a sharded phase whose step asks for it - the KV-split one, under the bounds
// check of sharded_self_attn.
static int fp8_self_attn(Ctx& c, int l, const void* q, void* o, int rows, int heads, int64_t q_rs, int64_t o_rs, int q_offset) {
  const rtv_dit_step* st = c.st;
  const rtv_attn_fp8_shadow* sh = c.fp8;
  const float scale = 1.0f / sqrtf((float)c.hd);
  const int S = st->attn_kv_splits;
  const int qo = st->causal_block > 0 ? q_offset : 0;
  const KeyWindow kw = key_window(st);
  if (S <= 1)
    return rtv_attn_fwd_fp8(q, sh->k8[l], sh->v8t[l], o, rows, heads, sh->cache_rows, kw.row0, kw.n0, kw.row1, kw.n1, q_rs, o_rs, scale,
                            sh->k_scale, sh->v_scale, st->causal_block, qo, c.stream);
  RTV_TRY(check_fp8_split(c, rows, heads));
  return rtv_attn_fwd_fp8_split(q, sh->k8[l], sh->v8t[l], o, rows, heads, sh->cache_rows, kw.row0, kw.n0, kw.row1, kw.n1, q_rs, o_rs,
                                scale, sh->k_scale, sh->v_scale, st->causal_block, qo, S, c.b.attn_part, c.b.attn_part_bytes, c.stream);
}

// ---- layer, part 2: attention over the cache window -> o-proj(+gate,+res) -> cross-attn -> FFN
static int dit_layer_rest(Ctx& c, int l) {
  const rtv_dit_step* st = c.st;
  DitBuffers& b = c.b;
  const int d = c.d, H = c.H, hd = c.hd, rc = c.rc, r0 = c.r0;
  rtv_stream_t stream = c.stream;
  const float scale = 1.0f / sqrtf((float)hd);
  const int64_t rs = st->kv_row_stride;
  const int Lkv = st->kv_hi - st->kv_lo;
  const int q_offset = st->cache_row0 - st->kv_lo + r0;  // position of local query row 0 inside the window
  uint16_t* kc = c.fp8_only ? nullptr : (uint16_t*)st->kv_k[l];
  uint16_t* vc = c.fp8_only ? nullptr : (uint16_t*)st->kv_v[l];
  // self attention (causal_model.py:386-390, :470-476)
  KeyWindow kw = key_window(st);
  if (c.fp8) {   // (rtv_dit_forward_attn_fp8: never sharded, never split; rtv_dit_layer_rest_attn_fp8: the local rows, maybe split)
    RTV_TRY(fp8_self_attn(c, l, b.q, b.ao, rc, H, d, d, q_offset));
  } else if (rc < c.M) {   // token-sharded call: the query grid is rc / 256 tiles per head - optionally cut along the keys
    RTV_TRY(sharded_self_attn(c, b.q, kc + (size_t)kw.row0 * rs, vc + (size_t)kw.row0 * rs, b.ao, rc, kw.n0, kw.n1,
                              kw.row1 - kw.row0, H, d, rs, d, q_offset));
  } else {
    RTV_TRY(rtv_attn_fwd_win(b.q, kc + (size_t)kw.row0 * rs, vc + (size_t)kw.row0 * rs, b.ao, 1, rc, kw.n0, kw.n1,
                             kw.row1 - kw.row0, H, hd, 0, d, 0, rs, 0, rs, 0, d, scale, st->causal_block,
                             st->causal_block > 0 ? q_offset : 0, RTV_DTYPE_BF16, stream));
  }
  (void)Lkv;
  if (void* qd = g_capture_q.load(std::memory_order_relaxed)) {   // test hook: this launch's operands, for a repeat outside the forward
    void* od = g_capture_o.load(std::memory_order_relaxed);
    const size_t bytes = (size_t)rc * d * sizeof(uint16_t);
    if (hipMemcpyAsync(qd, b.q, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess ||
        (od && hipMemcpyAsync(od, b.ao, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess))
      return set_error(-1, "dit: self-attention capture copy failed");
  }
  return dit_after_attn(c, l);
}

// ---- layer, part 3: b.ao (self-attention output of the local rows) -> o-proj(+gate,+res) -> cross-attn -> FFN
static int dit_after_attn(Ctx& c, int l) {
  const rtv_dit_layer_weights& lw = c.w->layers[l];
  const rtv_dit_step* st = c.st;
  DitBuffers& b = c.b;
  const int d = c.d, H = c.H, hd = c.hd, fs = c.fs, tc = c.tc, rc = c.rc, r0 = c.r0;
  rtv_stream_t stream = c.stream;
  const float eps = c.cfg->eps;
  const uint16_t* em = b.emod + (size_t)l * c.F * 6 * d;
  const float scale = 1.0f / sqrtf((float)hd);
  RTV_TRY(linear(c, S_LAYER0 + S_PER_LAYER * l + S_O, b.ao, d, lw.o_w, lw.o_b, b.x, rc, d, 0, em + 2 * d, 6 * d, fs, r0, b.x, tc, stream));
  // cross attention (causal_model.py:480, model.py:171-228)
  const void* ln_out = nullptr;
  RTV_TRY(ln_input(c, S_LAYER0 + S_PER_LAYER * l + S_CQ, nullptr, nullptr, 0, lw.norm3_w, lw.norm3_b, &ln_out));
  RTV_TRY(linear(c, S_LAYER0 + S_PER_LAYER * l + S_CQ, ln_out, d, lw.cq_w, lw.cq_b, b.qkv, rc, d, 0, nullptr, 0, 0, 0, nullptr, tc, stream));
  RTV_TRY(rtv_rmsnorm(b.qkv, d, b.q, d, rc, d, eps, lw.cnorm_q_w, stream));
  if (c.fold_k) {
    // short prompt: ao . Wo^T = sum_h P_h . (V_h . Wo_h^T) - the probabilities [rc][fold_k] go into b.ao, the projection multiplies
    // them by the folded weight made with the caches (K = fold_k instead of d; same epilogue)
    RTV_TRY(rtv_attn_probs_dup(b.q, st->ca_k[l], b.ao, rc, st->text_rows + 1, H, hd, d, d, c.fold_k, c.fold_kh, c.fold_k, scale,
                               st->text_rows, c.cfg->text_len - st->text_rows, stream));
    RTV_TRY(rtv_gemm(b.ao, c.fold_k, st->ca_v[c.L + l], st->ca_vo_ld, b.x, d, rc, d, c.fold_k, lw.co_b, 0, nullptr, 0, 0, 0, b.x, d,
                     RTV_DTYPE_BF16, tc, stream));
  } else {
    if (st->text_rows > 0 && st->text_rows + 1 < c.cfg->text_len)   // the padding rows share one K / V row: attend it once, weighted
      RTV_TRY(rtv_attn_fwd_dup(b.q, st->ca_k[l], st->ca_v[l], b.ao, 1, rc, st->text_rows + 1, H, hd, 0, d, 0, d, 0, d, 0, d, scale,
                               st->text_rows, c.cfg->text_len - st->text_rows, RTV_DTYPE_BF16, stream));
    else
      RTV_TRY(rtv_attn_fwd(b.q, st->ca_k[l], st->ca_v[l], b.ao, 1, rc, c.cfg->text_len, H, hd, 0, d, 0, d, 0, d, 0, d,
                           scale, 0, 0, RTV_DTYPE_BF16, stream));
    RTV_TRY(linear(c, S_LAYER0 + S_PER_LAYER * l + S_CO, b.ao, d, lw.co_w, lw.co_b, b.x, rc, d, 0, nullptr, 0, 0, 0, b.x, tc, stream));
  }
  // FFN (causal_model.py:482-488)
  RTV_TRY(ln_input(c, S_LAYER0 + S_PER_LAYER * l + S_FFN0, em + 3 * d, em + 4 * d, 6 * d, nullptr, nullptr, &ln_out));
  RTV_TRY(linear(c, S_LAYER0 + S_PER_LAYER * l + S_FFN0, ln_out, d, lw.ffn0_w, lw.ffn0_b, b.h, rc, c.ffn, RTV_ACT_GELU_TANH, nullptr, 0, 0, 0, nullptr, tc, stream));
  RTV_TRY(linear(c, S_LAYER0 + S_PER_LAYER * l + S_FFN2, b.h, c.ffn, lw.ffn2_w, lw.ffn2_b, b.x, rc, d, 0, em + 5 * d, 6 * d, fs, r0, b.x, tc, stream));
  return 0;
}

// ---- head-parallel phases.  Exchange buffers are caller-owned (the host runs the all-to-alls on them):
//   q_send  [world][rc][gc]       gc = (H/world)*128 columns of one head group
//   kv_send [world][rc][2][gc]    K and V of a row adjacent, i.e. the row layout of a K/V-interleaved cache arena
//   q_all / o_all [M][gc]         all query rows / attention output for this rank's heads
//   o_recv  [world][rc][gc]       attention output of the local rows, one block per head group
// In these phases step->kv_k / kv_v point at THIS RANK'S heads ([kv_size][H/world][128], row stride kv_row_stride).
static int hp_check(Ctx& c, int world) {
  // (world == 1 is the degenerate one-rank exchange: bench.py --cp-host-probe runs the whole head-parallel path on a one-rank group)
  if (world < 1 || c.H % world) return set_error(-1, "dit: head-parallel exchange needs num_heads % world == 0");
  if (c.M % world || c.rc != c.M / world || c.r0 % c.rc)
    return set_error(-1, "dit: head-parallel exchange needs equal token shards (M % world == 0)");
  return 0;
}

static int dit_layer_qkv_hp(Ctx& c, int l, int world, void* q_send, void* kv_send) {
  return dit_layer_proj(c, l, RTV_PROJ_LN | RTV_PROJ_Q | RTV_PROJ_KV, world, q_send, kv_send);
}

static int dit_layer_attn_hp(Ctx& c, int l, int world, const void* q_all, void* o_all) {
  RTV_TRY(hp_check(c, world));
  const rtv_dit_step* st = c.st;
  const int gc = c.d / world, hn = c.H / world;
  const int64_t rs = st->kv_row_stride;
  const int Lkv = st->kv_hi - st->kv_lo;
  const int q_offset = st->cache_row0 - st->kv_lo;
  const uint16_t* kc = (const uint16_t*)st->kv_k[l];
  const uint16_t* vc = (const uint16_t*)st->kv_v[l];
  KeyWindow kw = key_window(st);
  (void)Lkv;
  if (c.fp8) {   // rtv_dit_layer_attn_hp_attn_fp8: the exchange has delivered the block's rows of this rank's heads
    RTV_TRY(quantize_cache_rows(st, c.fp8, nullptr, l, st->cache_row0, c.M, hn, c.stream));
    return fp8_self_attn(c, l, q_all, o_all, c.M, hn, gc, gc, q_offset);
  }
  return sharded_self_attn(c, q_all, kc + (size_t)kw.row0 * rs, vc + (size_t)kw.row0 * rs, o_all, c.M, kw.n0, kw.n1,
                           kw.row1 - kw.row0, hn, gc, rs, gc, q_offset);
}

static int dit_layer_rest_hp(Ctx& c, int l, int world, const void* o_recv) {
  RTV_TRY(hp_check(c, world));
  RTV_TRY(regroup_heads(o_recv, c.b.ao, c.rc, world, c.d / world, c.stream));
  return dit_after_attn(c, l);
}

// ---- head on local rows (causal_model.py:512-523) -> head_rows[row_begin : row_begin+row_count)
static int dit_head(Ctx& c, void* head_rows) {
  DitBuffers& b = c.b;
  const int d = c.d, n = c.cfg->out_dim * 4;
  RTV_TRY(rtv_layernorm_modulate(b.x, b.xn, c.rc, d, c.cfg->eps, b.ehead + 0 * d, b.ehead + 1 * d, 2 * d, c.fs, c.r0, nullptr, nullptr, c.stream));
  RTV_TRY(linear(c, S_HEAD, b.xn, d, c.w->head_w, c.w->head_b, (uint16_t*)head_rows + (size_t)c.r0 * n, c.rc, n, 0, nullptr, 0, 0, 0, nullptr, c.tc, c.stream));
  return 0;
}

extern "C" int rtv_dit_begin(const rtv_dit_config* cfg, const rtv_dit_weights* w, const rtv_dit_step* st, void* ws,
                             size_t ws_bytes, rtv_stream_t stream) {
  Ctx c;
  RTV_TRY(make_ctx(cfg, w, st, ws, ws_bytes, stream, &c));
  return dit_begin(c);
}

extern "C" int rtv_dit_layer_qkv(const rtv_dit_config* cfg, const rtv_dit_weights* w, const rtv_dit_step* st, int layer,
                                 void* ws, size_t ws_bytes, rtv_stream_t stream) {
  Ctx c;
  RTV_TRY(make_ctx(cfg, w, st, ws, ws_bytes, stream, &c));
  if (layer < 0 || layer >= c.L) return set_error(-1, "dit: layer out of range");
  return dit_layer_qkv(c, layer);
}

extern "C" int rtv_dit_layer_proj(const rtv_dit_config* cfg, const rtv_dit_weights* w, const rtv_dit_step* st, int layer,
                                  int parts, int world, void* q_send, void* kv_send, void* ws, size_t ws_bytes,
                                  rtv_stream_t stream) {
  Ctx c;
  RTV_TRY(make_ctx(cfg, w, st, ws, ws_bytes, stream, &c));
  if (layer < 0 || layer >= c.L) return set_error(-1, "dit: layer out of range");
  return dit_layer_proj(c, layer, parts, world, q_send, kv_send);
}

extern "C" int rtv_dit_layer_rest(const rtv_dit_config* cfg, const rtv_dit_weights* w, const rtv_dit_step* st, int layer,
                                  void* ws, size_t ws_bytes, rtv_stream_t stream) {
  Ctx c;
  RTV_TRY(make_ctx(cfg, w, st, ws, ws_bytes, stream, &c));
  if (layer < 0 || layer >= c.L) return set_error(-1, "dit: layer out of range");
  return dit_layer_rest(c, layer);
}

extern "C" int rtv_dit_layer_qkv_hp(const rtv_dit_config* cfg, const rtv_dit_weights* w, const rtv_dit_step* st, int layer,
                                    int world, void* q_send, void* kv_send, void* ws, size_t ws_bytes, rtv_stream_t stream) {
  Ctx c;
  RTV_TRY(make_ctx(cfg, w, st, ws, ws_bytes, stream, &c));
  if (layer < 0 || layer >= c.L) return set_error(-1, "dit: layer out of range");
  if (!q_send || !kv_send) return set_error(-1, "dit: exchange buffers required");
  return dit_layer_qkv_hp(c, layer, world, q_send, kv_send);
}

extern "C" int rtv_dit_layer_attn_hp(const rtv_dit_config* cfg, const rtv_dit_weights* w, const rtv_dit_step* st, int layer,
                                     int world, const void* q_all, void* o_all, void* ws, size_t ws_bytes,
                                     rtv_stream_t stream) {
  Ctx c;
  RTV_TRY(make_ctx(cfg, w, st, ws, ws_bytes, stream, &c));
  if (layer < 0 || layer >= c.L) return set_error(-1, "dit: layer out of range");
  if (!q_all || !o_all) return set_error(-1, "dit: exchange buffers required");
  return dit_layer_attn_hp(c, layer, world, q_all, o_all);
}

extern "C" int rtv_dit_layer_rest_hp(const rtv_dit_config* cfg, const rtv_dit_weights* w, const rtv_dit_step* st, int layer,
                                     int world, const void* o_recv, void* ws, size_t ws_bytes, rtv_stream_t stream) {
  Ctx c;
  RTV_TRY(make_ctx(cfg, w, st, ws, ws_bytes, stream, &c));
  if (layer < 0 || layer >= c.L) return set_error(-1, "dit: layer out of range");
  if (!o_recv) return set_error(-1, "dit: exchange buffers required");
  return dit_layer_rest_hp(c, layer, world, o_recv);
}

extern "C" int rtv_dit_head(const rtv_dit_config* cfg, const rtv_dit_weights* w, const rtv_dit_step* st, void* head_rows,
                            void* ws, size_t ws_bytes, rtv_stream_t stream) {
  Ctx c;
  RTV_TRY(make_ctx(cfg, w, st, ws, ws_bytes, stream, &c));
  if (!head_rows) return set_error(-1, "dit: head_rows required");
  return dit_head(c, head_rows);
}

extern "C" int rtv_dit_finish(const rtv_dit_config* cfg, const rtv_dit_step* st, const void* head_rows,
                              rtv_stream_t stream) {
  if (!cfg || !st || !head_rows || !st->out) return set_error(-1, "dit: null argument");
  return rtv_unpatchify(head_rows, st->out, cfg->out_dim, st->F, st->gh, st->gw, stream);
}

// The e4m3-only cache: what its kernels and the attention launch would refuse layer by layer is refused here, in front of the first
// launch of the forward (nothing else holds the rows: a forward that fails half-way must not have overwritten codes).
static int check_fp8_only(const Ctx& c, const rtv_attn_fp8_shadow* sh) {
  const rtv_dit_step* st = c.st;
  for (int l = 0; l < c.L; ++l) {
    if (!sh->k8[l] || !sh->v8t[l]) return set_error(-1, "dit: fp8 attention: a layer has no shadow");
    if (((uintptr_t)sh->k8[l] | (uintptr_t)sh->v8t[l]) & 15) return set_error(-1, "dit: fp8 attention: k8 and v8t must be 16-byte aligned");
    if (sh->amax && ((uintptr_t)sh->amax[l] & 3)) return set_error(-1, "dit: fp8 attention: amax must be 4-byte aligned");
  }
  if (!(std::isfinite(sh->k_scale) && sh->k_scale > 0.f && std::isfinite(sh->v_scale) && sh->v_scale > 0.f))
    return set_error(-1, "dit: fp8 attention: scales must be finite and positive");
  // (make_ctx: the written rows lie inside the window, and the window inside the ring when there is one)
  const int64_t end = st->ring_size > 0 ? (int64_t)st->ring_lo + st->ring_size : (int64_t)st->kv_hi;
  if (end > sh->cache_rows) return set_error(-1, "dit: fp8 attention: the attention window lies outside [0, cache_rows)");
  int seg[3][2];
  return cut_written_rows(st, st->cache_row0, c.M, seg) < 0 ? -1 : 0;
}

// What the fp8 entry points ask of their shadow: need_shadow before anything else looks at the call (the four whole forwards),
// check_shadow where the arrays are first needed (dit_forward behind its context, the sharded phases).
static int need_shadow(const rtv_attn_fp8_shadow* shadow) {
  if (!shadow) return set_error(-1, "dit: fp8 attention needs its shadow (rtv_attn_fp8_shadow)");
  return 0;
}
static int check_shadow(const rtv_attn_fp8_shadow* shadow) {
  RTV_TRY(need_shadow(shadow));
  if (!shadow->k8 || !shadow->v8t || shadow->cache_rows <= 0)
    return set_error(-1, "dit: fp8 attention needs the k8 / v8t shadow arrays and cache_rows");
  return 0;
}

// The unsharded composition; fp8 != null: self-attention on the e4m3 shadows (rtv_dit_forward_attn_fp8), centers != null: whose K
// codes are centred (rtv_dit_forward_attn_fp8_centered); fp8_only: whose shadows are the whole cache (rtv_dit_forward_attn_fp8_only;
// with centers: rtv_dit_forward_attn_fp8_only_centered).
static int dit_forward(const rtv_dit_config* cfg, const rtv_dit_weights* w, const rtv_dit_step* st, const rtv_attn_fp8_shadow* fp8,
                       void* const* centers, bool fp8_only, void* workspace, size_t workspace_bytes, rtv_stream_t stream) {
  Ctx c;
  RTV_TRY(make_ctx(cfg, w, st, workspace, workspace_bytes, stream, &c));
  if (fp8) {
    // sharded and split steps have phases of their own (rtv_hip_attn_fp8_cp.h); handed to THIS entry point they are refused -
    // never a bf16 run in their place
    if (c.r0 != 0 || c.rc != c.M) return set_error(-1, "dit: fp8 attention does not support sharded calls (row_count < M)");
    if (st->attn_kv_splits > 1) return set_error(-1, "dit: fp8 attention does not support attn_kv_splits > 1");
    RTV_TRY(check_shadow(fp8));
    if (centers)
      for (int l = 0; l < c.L; ++l) {
        if (!centers[l]) return set_error(-1, "dit: fp8 attention: a layer has no K centre");
        // (the shadow mode's quantiser makes this check layer by layer; the compact cache has nothing to derive its rows from again)
        if (fp8_only && ((uintptr_t)centers[l] & 15)) return set_error(-1, "dit: fp8 attention: a K centre must be 16-byte aligned");
      }
    if (fp8_only) RTV_TRY(check_fp8_only(c, fp8));
    c.fp8 = fp8;
    c.centers = centers;
    c.fp8_only = fp8_only;
  }
  if (c.r0 != 0 || c.rc != c.M)
    return set_error(-1, "dit_forward: sharded row ranges need the phase API (rtv_dit_begin/layer_qkv/layer_rest/head/finish)");
  RTV_TRY(dit_begin(c));
  for (int l = 0; l < c.L; ++l) {
    if (st->kv_only && l == c.L - 1)   // nothing downstream of the last layer's K / V rows is consumed
      return dit_layer_proj(c, l, RTV_PROJ_LN | RTV_PROJ_KV, 0, nullptr, nullptr);
    RTV_TRY(dit_layer_qkv(c, l));
    RTV_TRY(dit_layer_rest(c, l));
  }
  RTV_TRY(dit_head(c, c.b.hrow));
  return rtv_unpatchify(c.b.hrow, st->out, cfg->out_dim, c.F, c.gh, c.gw, stream);
}

extern "C" int rtv_dit_forward(const rtv_dit_config* cfg, const rtv_dit_weights* w, const rtv_dit_step* st,
                               void* workspace, size_t workspace_bytes, rtv_stream_t stream) {
  return dit_forward(cfg, w, st, nullptr, nullptr, false, workspace, workspace_bytes, stream);
}

extern "C" int rtv_dit_forward_attn_fp8(const rtv_dit_config* cfg, const rtv_dit_weights* w, const rtv_dit_step* st,
                                        const rtv_attn_fp8_shadow* shadow, void* workspace, size_t workspace_bytes,
                                        rtv_stream_t stream) {
  RTV_TRY(need_shadow(shadow));
  return dit_forward(cfg, w, st, shadow, nullptr, false, workspace, workspace_bytes, stream);
}

extern "C" int rtv_dit_forward_attn_fp8_centered(const rtv_dit_config* cfg, const rtv_dit_weights* w, const rtv_dit_step* st,
                                                 const rtv_attn_fp8_shadow* shadow, void* const* centers, void* workspace,
                                                 size_t workspace_bytes, rtv_stream_t stream) {
  RTV_TRY(need_shadow(shadow));
  if (!centers) return set_error(-1, "dit: centred fp8 attention needs its table of K centres");
  return dit_forward(cfg, w, st, shadow, centers, false, workspace, workspace_bytes, stream);
}

extern "C" int rtv_dit_forward_attn_fp8_only(const rtv_dit_config* cfg, const rtv_dit_weights* w, const rtv_dit_step* st,
                                             const rtv_attn_fp8_shadow* shadow, void* workspace, size_t workspace_bytes,
                                             rtv_stream_t stream) {
  RTV_TRY(need_shadow(shadow));
  return dit_forward(cfg, w, st, shadow, nullptr, true, workspace, workspace_bytes, stream);
}

extern "C" int rtv_dit_forward_attn_fp8_only_centered(const rtv_dit_config* cfg, const rtv_dit_weights* w, const rtv_dit_step* st,
                                                      const rtv_attn_fp8_shadow* shadow, void* const* centers, void* workspace,
                                                      size_t workspace_bytes, rtv_stream_t stream) {
  RTV_TRY(need_shadow(shadow));
  if (!centers) return set_error(-1, "dit: centred fp8 attention needs its table of K centres");
  return dit_forward(cfg, w, st, shadow, centers, true, workspace, workspace_bytes, stream);
}

// ---- the sharded phases with the self-attention in fp8 (rtv_hip_attn_fp8_cp.h)
extern "C" int rtv_dit_quantize_block_attn_fp8(const rtv_dit_config* cfg, const rtv_dit_step* st, int layer, int heads,
                                               const rtv_attn_fp8_shadow* shadow, rtv_stream_t stream) {
  if (!cfg || !st) return set_error(-1, "dit: null argument");
  RTV_TRY(check_shadow(shadow));
  if (layer < 0 || layer >= cfg->num_layers) return set_error(-1, "dit: layer out of range");
  if (heads <= 0 || heads > cfg->num_heads) return set_error(-1, "dit: fp8 attention: heads must be 1..num_heads");
  const int64_t M = (int64_t)st->F * st->gh * st->gw;
  if (st->F <= 0 || st->gh <= 0 || st->gw <= 0 || M > INT32_MAX) return set_error(-1, "dit: empty token grid");
  if (!st->kv_k || !st->kv_v || !st->kv_k[layer] || !st->kv_v[layer]) return set_error(-1, "dit: null argument");
  if (st->cache_row0 < 0 || st->ring_size < 0 || st->ring_lo < 0 || st->ring_shift < 0 ||
      (st->ring_size > 0 && st->ring_shift >= st->ring_size) || (st->ring_size > 0 && st->cache_row0 + M > st->ring_lo + st->ring_size))
    return set_error(-1, "dit: bad ring window (0 <= ring_shift < ring_size, kv_hi <= ring_lo + ring_size)");
  return quantize_cache_rows(st, shadow, nullptr, layer, st->cache_row0, (int)M, heads, stream);
}

extern "C" int rtv_dit_layer_rest_attn_fp8(const rtv_dit_config* cfg, const rtv_dit_weights* w, const rtv_dit_step* st, int layer,
                                           const rtv_attn_fp8_shadow* shadow, void* ws, size_t ws_bytes, rtv_stream_t stream) {
  Ctx c;
  RTV_TRY(make_ctx(cfg, w, st, ws, ws_bytes, stream, &c));
  if (layer < 0 || layer >= c.L) return set_error(-1, "dit: layer out of range");
  RTV_TRY(check_shadow(shadow));
  c.fp8 = shadow;
  RTV_TRY(check_fp8_split(c, c.rc, c.H));
  RTV_TRY(quantize_cache_rows(st, shadow, nullptr, layer, st->cache_row0, c.M, c.H, stream));   // the gathered rows, every rank for itself
  return dit_layer_rest(c, layer);
}

extern "C" int rtv_dit_layer_attn_hp_attn_fp8(const rtv_dit_config* cfg, const rtv_dit_weights* w, const rtv_dit_step* st, int layer,
                                              int world, const void* q_all, void* o_all, const rtv_attn_fp8_shadow* shadow, void* ws,
                                              size_t ws_bytes, rtv_stream_t stream) {
  Ctx c;
  RTV_TRY(make_ctx(cfg, w, st, ws, ws_bytes, stream, &c));
  if (layer < 0 || layer >= c.L) return set_error(-1, "dit: layer out of range");
  if (!q_all || !o_all) return set_error(-1, "dit: exchange buffers required");
  RTV_TRY(check_shadow(shadow));
  c.fp8 = shadow;
  RTV_TRY(hp_check(c, world));
  RTV_TRY(check_fp8_split(c, c.M, c.H / world));
  return dit_layer_attn_hp(c, layer, world, q_all, o_all);
}

// ---- the e4m3-only cache under the row exchange: the exchange carries codes (rtv_hip_attn_fp8_only_cp.h)
// What the three phases ask of the staging buffer and of the step's rows before anything is launched.
static int check_kv8(const void* kv8, int world, int M) {
  if (!kv8) return set_error(-1, "dit: fp8 attention: the code exchange needs its staging buffer kv8");
  if ((uintptr_t)kv8 & 15) return set_error(-1, "dit: fp8 attention: kv8 must be 16-byte aligned");
  if (world <= 0 || M % world) return set_error(-1, "dit: fp8 attention: M = F * gh * gw must be a multiple of world");
  return 0;
}

// One layer's arrays and the scales, as check_fp8_only asks them of every layer.
static int check_fp8_only_layer(const rtv_attn_fp8_shadow* sh, int l) {
  if (!sh->k8[l] || !sh->v8t[l]) return set_error(-1, "dit: fp8 attention: a layer has no shadow");
  if (((uintptr_t)sh->k8[l] | (uintptr_t)sh->v8t[l]) & 15) return set_error(-1, "dit: fp8 attention: k8 and v8t must be 16-byte aligned");
  if (sh->amax && ((uintptr_t)sh->amax[l] & 3)) return set_error(-1, "dit: fp8 attention: amax must be 4-byte aligned");
  if (!(std::isfinite(sh->k_scale) && sh->k_scale > 0.f && std::isfinite(sh->v_scale) && sh->v_scale > 0.f))
    return set_error(-1, "dit: fp8 attention: scales must be finite and positive");
  return 0;
}

extern "C" int rtv_dit_layer_proj_attn_fp8_only(const rtv_dit_config* cfg, const rtv_dit_weights* w, const rtv_dit_step* st, int layer,
                                                int parts, int world, void* kv8, const rtv_attn_fp8_shadow* shadow, void* ws,
                                                size_t ws_bytes, rtv_stream_t stream) {
  Ctx c;
  RTV_TRY(make_ctx(cfg, w, st, ws, ws_bytes, stream, &c));
  if (layer < 0 || layer >= c.L) return set_error(-1, "dit: layer out of range");
  RTV_TRY(check_shadow(shadow));
  RTV_TRY(check_fp8_only_layer(shadow, layer));
  RTV_TRY(check_kv8(kv8, world, c.M));
  const int S = c.M / world;
  if (c.r0 / S != (c.r0 + c.rc - 1) / S) return set_error(-1, "dit: fp8 attention: the local rows must lie in one rank's segment of kv8");
  c.fp8 = shadow;
  c.fp8_only = true;
  c.kv8 = kv8;
  c.kv8_world = world;
  return dit_layer_proj(c, layer, parts, 0, nullptr, nullptr);
}

static int commit_block_fp8_only(const rtv_dit_step* st, int M, int H, int layer, int world, const void* kv8,
                                 const rtv_attn_fp8_shadow* sh, rtv_stream_t stream) {
  return rtv_attn_fp8_commit_kv8(kv8, world, M, H, sh->k8[layer], sh->v8t[layer], sh->cache_rows, st->cache_row0, st->ring_lo,
                                 st->ring_size, st->ring_shift, stream);
}

extern "C" int rtv_dit_commit_block_attn_fp8_only(const rtv_dit_config* cfg, const rtv_dit_step* st, int layer, int world,
                                                  const void* kv8, const rtv_attn_fp8_shadow* shadow, rtv_stream_t stream) {
  if (!cfg || !st) return set_error(-1, "dit: null argument");
  RTV_TRY(check_shadow(shadow));
  if (layer < 0 || layer >= cfg->num_layers) return set_error(-1, "dit: layer out of range");
  RTV_TRY(check_fp8_only_layer(shadow, layer));
  const int64_t M = (int64_t)st->F * st->gh * st->gw;
  if (st->F <= 0 || st->gh <= 0 || st->gw <= 0 || M > INT32_MAX) return set_error(-1, "dit: empty token grid");
  RTV_TRY(check_kv8(kv8, world, (int)M));
  return commit_block_fp8_only(st, (int)M, cfg->num_heads, layer, world, kv8, shadow, stream);
}

extern "C" int rtv_dit_layer_rest_attn_fp8_only(const rtv_dit_config* cfg, const rtv_dit_weights* w, const rtv_dit_step* st, int layer,
                                                int world, const void* kv8, const rtv_attn_fp8_shadow* shadow, void* ws,
                                                size_t ws_bytes, rtv_stream_t stream) {
  Ctx c;
  RTV_TRY(make_ctx(cfg, w, st, ws, ws_bytes, stream, &c));
  if (layer < 0 || layer >= c.L) return set_error(-1, "dit: layer out of range");
  RTV_TRY(check_shadow(shadow));
  RTV_TRY(check_fp8_only_layer(shadow, layer));
  RTV_TRY(check_kv8(kv8, world, c.M));
  // (make_ctx: the written rows lie inside the window, and the window inside the ring when there is one)
  const int64_t end = st->ring_size > 0 ? (int64_t)st->ring_lo + st->ring_size : (int64_t)st->kv_hi;
  if (end > shadow->cache_rows) return set_error(-1, "dit: fp8 attention: the attention window lies outside [0, cache_rows)");
  c.fp8 = shadow;
  c.fp8_only = true;
  RTV_TRY(check_fp8_split(c, c.rc, c.H));
  RTV_TRY(commit_block_fp8_only(st, c.M, c.H, layer, world, kv8, shadow, stream));   // the gathered codes, every rank for itself
  return dit_layer_rest(c, layer);
}

extern "C" int rtv_dit_lab_capture_self_attn(void* q_copy, void* o_copy) {
  g_capture_q = q_copy;
  g_capture_o = o_copy;
  return 0;
}

extern "C" int rtv_dit_set_direct_v(int on) {
  g_direct_v = on ? 1 : 0;
  return 0;
}
