// The JPEG decoder's core, shared by the kernels (jpeg_decode.hip) and by a stand-alone host program (jpeg_decode_hostcheck.cpp)
// that emulates the kernels' rounds serially and is what damaged files are run through first, under the sanitizers, on the CPU:
// the host parser, the bit reader, the table lookup, the per-symbol state machine with its bounds checks, the block layout, and
// the integer arithmetic of the pixel stage (libjpeg's islow IDCT, range limit and colour tables).  Plain C++, no HIP type.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/rtv_hip_jpeg_decode.h"

#if defined(__HIPCC__)
#define JD_HD __host__ __device__ __forceinline__
#else
#define JD_HD inline
#endif

namespace rtv {
namespace jd {

struct Huff {                 // rtv_jpeg_desc::huff[i], see include/rtv_hip_jpeg_decode.h
  uint16_t fast[256];
  uint32_t limit[17];
  int32_t offs[17];
  uint8_t vals[256];
  uint32_t pad[2];
};
static_assert(sizeof(Huff) == RTV_JPEG_HUFF_WORDS * 4, "Huff is RTV_JPEG_HUFF_WORDS words");
static_assert(sizeof(rtv_jpeg_desc) == 4496 && sizeof(rtv_jpeg_desc) % 16 == 0, "rtv_jpeg_desc is 4496 bytes");

constexpr int SUBSEQ_BITS_DEFAULT = 512;
constexpr int MAX_SUBSEQ = 1024;          // subsequences of a scan = threads of the entropy workgroup

// zigzag index -> natural (row-major) index, T.81 figure A.6
#define JD_NATURAL_ORDER                                                                                                     \
  {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, \
   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

// ------------------------------------------------------------------------------------------------------------- geometry, layout
struct Geom {                 // what the kernels need of a descriptor besides the tables; checked by geom_from_desc
  int H, W, ncomp, hs, vs, ri, mcu_cols, mcu_rows, bpm;
  int scan_offset, scan_bytes;
  JD_HD int total_blocks() const { return mcu_cols * mcu_rows * bpm; }
  JD_HD int grid_w(int c) const { return c ? mcu_cols : mcu_cols * hs; }
  JD_HD int grid_h(int c) const { return c ? mcu_rows : mcu_rows * vs; }
  JD_HD int plane_offset(int c) const {   // in int16 elements: component after component
    int o = 0;
    for (int k = 0; k < c; ++k) o += grid_w(k) * grid_h(k) * 64;
    return o;
  }
  JD_HD int coef_elems() const { return plane_offset(ncomp); }
  JD_HD int slot_comp(int slot) const { return slot < hs * vs ? 0 : slot - hs * vs + 1; }
  // block `slot` of MCU `mcu` (scan order: the luma blocks row by row, then Cb, then Cr) -> its first element in the planes
  JD_HD int block_offset(int mcu, int slot) const {
    const int my = mcu / mcu_cols, mx = mcu - my * mcu_cols;
    const int c = slot_comp(slot);
    if (c == 0) {
      const int sy = slot / hs, sx = slot - sy * hs;
      return ((my * vs + sy) * (mcu_cols * hs) + mx * hs + sx) * 64;
    }
    return plane_offset(c) + (my * mcu_cols + mx) * 64;
  }
};

// null = fine, else why the descriptor cannot be decoded (fields that contradict each other or exceed the caps)
inline const char* geom_from_desc(const rtv_jpeg_desc& d, Geom* g) {
  if (d.height < 1 || d.width < 1 || d.height > RTV_JPEG_DECODE_MAX_SIDE || d.width > RTV_JPEG_DECODE_MAX_SIDE)
    return "descriptor: width and height must be in 1..4096";
  if (d.components != 1 && d.components != 3) return "descriptor: 1 or 3 components";
  const bool ok_samp = (d.hsamp == 1 && d.vsamp == 1) || (d.components == 3 && d.hsamp == 2 && (d.vsamp == 1 || d.vsamp == 2));
  if (!ok_samp) return "descriptor: luma sampling must be 1x1, 2x1 or 2x2";
  if (d.mcu_cols != (d.width + 8 * d.hsamp - 1) / (8 * d.hsamp) || d.mcu_rows != (d.height + 8 * d.vsamp - 1) / (8 * d.vsamp) ||
      d.blocks_per_mcu != d.hsamp * d.vsamp + d.components - 1)
    return "descriptor: the MCU grid does not follow from the sizes";
  if (d.restart_interval < 0 || d.restart_interval > 65535) return "descriptor: restart interval outside 0..65535";
  if (d.file_bytes < 1 || d.file_bytes > RTV_JPEG_DECODE_MAX_FILE || d.scan_offset < 0 || d.scan_bytes < 0 ||
      d.scan_offset > d.file_bytes || d.scan_bytes > d.file_bytes - d.scan_offset)
    return "descriptor: the scan does not lie inside the file";
  for (int c = 0; c < d.components; ++c)
    if (d.comp_dc[c] < 0 || d.comp_dc[c] > 1 || d.comp_ac[c] < 2 || d.comp_ac[c] > 3) return "descriptor: table slots out of range";
  *g = Geom{d.height, d.width, d.components, d.hsamp, d.vsamp, d.restart_interval, d.mcu_cols, d.mcu_rows, d.blocks_per_mcu,
            d.scan_offset, d.scan_bytes};
  return nullptr;
}

// bits of a subsequence for a scan of scan_bytes: the asked length (0 = default), raised until MAX_SUBSEQ subsequences cover it
JD_HD int effective_subseq_bits(int asked, int scan_bytes) {
  int L = asked > 0 ? asked : SUBSEQ_BITS_DEFAULT;
  const long long bits = (long long)scan_bytes * 8;
  const long long need = (bits + MAX_SUBSEQ - 1) / MAX_SUBSEQ;
  if (need > L) L = (int)((need + 31) / 32 * 32);
  return L;
}

// ------------------------------------------------------------------------------------------------------------------ host parser
namespace parse_detail {
inline bool build_huff(const uint8_t* bits, const uint8_t* vals, int nvals, Huff* h) {   // T.81 Annex C; false = malformed
  memset(h, 0, sizeof(*h));
  for (int i = 0; i < nvals; ++i) h->vals[i] = vals[i];
  uint32_t code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    h->offs[l] = k - (int)code;
    for (int i = 0; i < bits[l - 1]; ++i, ++k, ++code) {
      if (code >= (1u << l)) return false;                       // more codes than the length has
      if (l <= 8)
        for (uint32_t f = code << (8 - l); f < ((code + 1) << (8 - l)); ++f) h->fast[f] = (uint16_t)((l << 8) | vals[k]);
    }
    if (code > (1u << l)) return false;
    h->limit[l] = code << (16 - l);
    code <<= 1;
  }
  return true;
}
}  // namespace parse_detail

// null = parsed into *d, else the reason for the refusal.  Reads file[0 .. n) only.
inline const char* parse(const uint8_t* f, size_t n, rtv_jpeg_desc* d) {
  using parse_detail::build_huff;
  static const uint8_t natural[64] = JD_NATURAL_ORDER;
  if (n > RTV_JPEG_DECODE_MAX_FILE) return "file above the 8 MiB cap";
  if (n < 4 || f[0] != 0xFF || f[1] != 0xD8) return "not a JPEG file (no SOI marker)";
  memset(d, 0, sizeof(*d));
  int qt[4][64];
  bool have_qt[4] = {false, false, false, false}, have_huff[4] = {false, false, false, false};
  bool have_sof = false, adobe = false;
  int adobe_transform = -1, comp_id[3] = {0, 0, 0}, comp_tq[3] = {0, 0, 0}, comp_h[3] = {1, 1, 1}, comp_v[3] = {1, 1, 1};
  size_t at = 2;
  for (;;) {
    if (at + 2 > n) return "truncated header (the file ends before the scan)";
    if (f[at] != 0xFF) return "malformed header (a marker was expected)";
    const int m = f[at + 1];
    if (m == 0xFF) {                                             // fill byte
      ++at;
      continue;
    }
    at += 2;
    if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;   // parameterless
    if (m == 0xD9) return "no scan (EOI before SOS)";
    if (at + 2 > n) return "truncated header (the file ends inside a marker segment)";
    const size_t len = ((size_t)f[at] << 8) | f[at + 1];
    if (len < 2 || at + len > n) return "truncated header (the file ends inside a marker segment)";
    const uint8_t* p = f + at + 2;
    const size_t pl = len - 2;
    if (m == 0xC0) {
      if (have_sof) return "malformed header (two frame headers)";
      if (pl < 6) return "malformed header (SOF0 too short)";
      if (p[0] == 12) return "12-bit samples are not supported";
      if (p[0] != 8) return "sample precision must be 8 bits";
      d->height = (p[1] << 8) | p[2];
      d->width = (p[3] << 8) | p[4];
      d->components = p[5];
      if (d->components == 4) return "4 components (CMYK / YCCK) are not supported";
      if (d->components != 1 && d->components != 3) return "only 1 or 3 components are supported";
      if (pl < 6 + 3 * (size_t)d->components) return "malformed header (SOF0 too short)";
      if (d->height < 1 || d->width < 1) return "width and height must be positive";
      if (d->height > RTV_JPEG_DECODE_MAX_SIDE || d->width > RTV_JPEG_DECODE_MAX_SIDE) return "width or height above the 4096 cap";
      for (int c = 0; c < d->components; ++c) {
        comp_id[c] = p[6 + 3 * c];
        comp_h[c] = p[7 + 3 * c] >> 4;
        comp_v[c] = p[7 + 3 * c] & 15;
        comp_tq[c] = p[8 + 3 * c];
        if (comp_tq[c] > 3) return "malformed header (quantisation table id above 3)";
      }
      if (d->components == 1) {
        d->hsamp = d->vsamp = 1;                                  // a one-component scan is not interleaved: one block per MCU
      } else {
        d->hsamp = comp_h[0];
        d->vsamp = comp_v[0];
        const bool luma_ok = (d->hsamp == 1 && d->vsamp == 1) || (d->hsamp == 2 && (d->vsamp == 1 || d->vsamp == 2));
        if (!luma_ok || comp_h[1] != 1 || comp_v[1] != 1 || comp_h[2] != 1 || comp_v[2] != 1)
          return "sampling factors other than 4:4:4, 4:2:2 (2x1) and 4:2:0 (2x2) are not supported";
      }
      have_sof = true;
    } else if ((m >= 0xC1 && m <= 0xCF) && m != 0xC4 && m != 0xC8 && m != 0xCC) {
      if (m == 0xC2) return "progressive JPEG is not supported";
      if (m == 0xC1) return "extended sequential JPEG is not supported";
      if (m == 0xC3 || m == 0xC7 || m == 0xCB || m == 0xCF) return "lossless JPEG is not supported";
      if (m >= 0xC9) return "arithmetic coding is not supported";
      return "differential (hierarchical) JPEG is not supported";
    } else if (m == 0xCC) {
      return "arithmetic coding is not supported";
    } else if (m == 0xC4) {
      size_t o = 0;
      while (o < pl) {
        if (o + 17 > pl) return "malformed header (DHT cut short)";
        const int tc = p[o] >> 4, th = p[o] & 15;
        if (tc > 1 || th > 1) return "Huffman table class / id outside what baseline allows (0 and 1)";
        int count = 0;
        for (int i = 0; i < 16; ++i) count += p[o + 1 + i];
        if (count > 256 || o + 17 + count > pl) return "malformed header (DHT cut short)";
        if (!build_huff(p + o + 1, p + o + 17, count, (Huff*)d->huff[tc * 2 + th])) return "malformed Huffman table";
        have_huff[tc * 2 + th] = true;
        o += 17 + count;
      }
    } else if (m == 0xDB) {
      size_t o = 0;
      while (o < pl) {
        const int pq = p[o] >> 4, tq = p[o] & 15;
        if (pq == 1) return "16-bit quantisation tables are not supported";
        if (pq != 0 || tq > 3) return "malformed header (DQT)";
        if (o + 65 > pl) return "malformed header (DQT cut short)";
        for (int i = 0; i < 64; ++i) qt[tq][natural[i]] = p[o + 1 + i];
        have_qt[tq] = true;
        o += 65;
      }
    } else if (m == 0xDD) {
      if (pl < 2) return "malformed header (DRI)";
      d->restart_interval = (p[0] << 8) | p[1];
    } else if (m == 0xEE) {
      if (pl >= 12 && memcmp(p, "Adobe", 5) == 0) {
        adobe = true;
        adobe_transform = p[11];
      }
    } else if (m == 0xDA) {
      if (!have_sof) return "malformed header (SOS before SOF0)";
      if (pl < 1 || p[0] != d->components) return "more than one scan (the scan does not hold every component)";
      if (pl < 4 + 2 * (size_t)d->components) return "malformed header (SOS too short)";
      for (int c = 0; c < d->components; ++c) {
        if (p[1 + 2 * c] != comp_id[c]) return "malformed header (scan components out of order)";
        const int td = p[2 + 2 * c] >> 4, ta = p[2 + 2 * c] & 15;
        if (td > 1 || ta > 1) return "Huffman table id outside what baseline allows (0 and 1)";
        if (!have_huff[td] || !have_huff[2 + ta]) return "missing Huffman table (the scan names one the file does not define)";
        if (!have_qt[comp_tq[c]]) return "missing quantisation table";
        d->comp_dc[c] = td;
        d->comp_ac[c] = 2 + ta;
        for (int i = 0; i < 64; ++i) d->quant[c][i] = qt[comp_tq[c]][i];
      }
      const uint8_t* t = p + 1 + 2 * d->components;
      if (t[0] != 0 || t[1] != 63 || t[2] != 0) return "more than one scan (spectral selection / successive approximation)";
      if (adobe && d->components == 3 && adobe_transform == 0) return "Adobe APP14 transform 0 (RGB, not Y Cb Cr) is not supported";
      at += len;
      break;
    }
    at += len;
  }
  d->mcu_cols = (d->width + 8 * d->hsamp - 1) / (8 * d->hsamp);
  d->mcu_rows = (d->height + 8 * d->vsamp - 1) / (8 * d->vsamp);
  d->blocks_per_mcu = d->hsamp * d->vsamp + d->components - 1;
  d->file_bytes = (int)n;
  d->scan_offset = (int)at;
  // the scan ends at the first marker that is no restart marker (0xFF 0x00 is a stuffed data byte, 0xFF 0xFF a fill byte)
  size_t e = at;
  int marker = -1;
  while (e < n) {
    const uint8_t* q = (const uint8_t*)memchr(f + e, 0xFF, n - e);
    if (!q) {
      e = n;
      break;
    }
    e = (size_t)(q - f);
    if (e + 1 >= n) {
      e = n;
      break;
    }
    const int b = f[e + 1];
    if (b == 0x00 || b == 0xFF || (b >= 0xD0 && b <= 0xD7)) {
      e += b == 0xFF ? 1 : 2;
      continue;
    }
    marker = b;
    break;
  }
  if (marker == 0xDA || marker == 0xC4 || marker == 0xDB || marker == 0xDD || (marker >= 0xC0 && marker <= 0xCF))
    return "more than one scan";
  d->scan_bytes = (int)(e - at);
  return nullptr;
}

// ------------------------------------------------------------------------------------------------------------------- bit reader
// MSB-first reader of the stuffed scan s[0 .. n): a 0x00 behind a 0xFF is skipped as it is met (no pass over the file), any other
// byte behind a 0xFF is a marker and stops the reader in front of it, as does the end of the scan.  It never reads s[n] or beyond.
struct Reader {
  const uint8_t* s;
  uint32_t n;
  uint32_t pos;               // next byte to load
  uint64_t acc;               // the low `cnt` bits are the next unread bits
  int cnt;
  bool stopped;               // a marker or the end of the scan is at `pos`
  JD_HD void start(const uint8_t* scan, uint32_t len, uint32_t bit) {
    s = scan, n = len, pos = bit >> 3, acc = 0, cnt = 0, stopped = false;
    if (pos > n) pos = n;
    const int skip = (int)(bit & 7);
    if (skip) {
      fill();
      if (cnt >= 8) cnt -= skip;   // else the position lies at the end or on a marker: nothing to skip
    }
  }
  JD_HD void fill() {
    while (cnt <= 56 && !stopped) {
      if (pos >= n) {
        stopped = true;
        break;
      }
      const uint32_t b = s[pos];
      if (b == 0xFF) {
        if (pos + 1 >= n || s[pos + 1] != 0x00) {
          stopped = true;
          break;
        }
        pos += 2;
      } else {
        ++pos;
      }
      acc = (acc << 8) | b;
      cnt += 8;
    }
  }
  // the next k <= 16 bits, zero-filled behind the last real bit
  JD_HD uint32_t peek(int k) {
    if (cnt < k) fill();
    if (cnt >= k) return (uint32_t)(acc >> (cnt - k)) & ((1u << k) - 1u);
    return (uint32_t)(acc << (k - cnt)) & ((1u << k) - 1u);
  }
  JD_HD void drop(int k) { cnt -= k; }   // the caller has checked k <= cnt
  // an upper bound of the position of the next unread bit (exact when no stuffed byte lies among the buffered ones)
  JD_HD uint32_t bound() const { return pos * 8u - (uint32_t)cnt; }
  // the exact position of the next unread bit: the buffered bits walked back over the bytes they came from
  JD_HD uint32_t position() const {
    uint32_t p = pos;
    int k = cnt;
    while (k > 0 && p > 0) {
      --p;
      if (s[p] == 0x00 && p > 0 && s[p - 1] == 0xFF) --p;      // the stuffed byte behind a data 0xFF
      if (k <= 8) return p * 8u + (uint32_t)(8 - k);
      k -= 8;
    }
    return p * 8u;
  }
  // the marker the reader stopped at: 0xD0..0xD7, another marker byte, or -1 for the end of the scan
  JD_HD int marker() const { return (pos + 1 < n && s[pos] == 0xFF) ? (int)s[pos + 1] : -1; }
  JD_HD void jump_marker() { pos += 2, acc = 0, cnt = 0, stopped = false; }
};

// ---------------------------------------------------------------------------------------------------------------- state machine
struct State {                // where a decoder stands between two symbols
  uint32_t bit;               // position of the next unread bit in the stuffed scan; END_BIT = the scan is over
  uint32_t aux;               // zigzag index of the next coefficient (0 = a DC term comes) | block slot within the MCU << 8
  JD_HD bool operator==(const State& o) const { return bit == o.bit && aux == o.aux; }
};
constexpr uint32_t END_BIT = 0xFFFFFFFFu;

struct Counts {               // what a subsequence adds to the block count: (c, n) = c restart markers crossed, n blocks completed
  int c, n;                   // since the last of them (since the subsequence's start if c == 0)
};
JD_HD Counts combine(Counts a, Counts b) { return b.c ? Counts{a.c + b.c, b.n} : Counts{a.c, a.n + b.n}; }

// Sink of the final pass: knows the absolute block index at the subsequence's start and writes coefficients to their places.
struct Counts;
struct NullSink {
  JD_HD void put(int, int, int, int, int) {}
  JD_HD void at_marker(Counts) {}
};
struct CoefSink {
  int16_t* coef;
  const uint8_t* natural;
  Geom g;
  Counts base;                // the counts in front of this subsequence
  int status;                 // RTV_JPEG_STATUS_BLOCKS / _MARKER found by the index checks
  int reached;                // one past the highest block index written to
  // absolute index of the block that is `k.n` blocks behind the last marker; -1 where it must not be written
  JD_HD int index(Counts k) {
    const Counts t = combine(base, k);
    if (g.ri > 0 && t.n >= g.ri * g.bpm) {
      status |= RTV_JPEG_STATUS_BLOCKS;
      return -1;
    }
    const long long b = (long long)t.c * g.ri * g.bpm + t.n;
    if (b >= g.total_blocks()) {
      status |= RTV_JPEG_STATUS_BLOCKS;
      return -1;
    }
    return (int)b;
  }
  JD_HD void put(int c, int n, int slot, int zz, int v) {
    const int b = index(Counts{c, n});
    if (b < 0) return;
    if (b + 1 > reached) reached = b + 1;
    coef[g.block_offset(b / g.bpm, slot) + natural[zz & 63]] = (int16_t)v;
  }
  // a restart marker is crossed after k: it belongs behind exactly ri MCUs
  JD_HD void at_marker(Counts k) {
    const Counts t = combine(base, k);
    if (t.n != g.ri * g.bpm) status |= RTV_JPEG_STATUS_MARKER;
  }
};

struct Tables {
  const Huff* huff;           // [4]
  const uint8_t* natural;     // [64]
  uint32_t select;            // bit c: the DC table of component c; bit 4 + c: its AC table (no array: nothing to index per thread)
  JD_HD void set(const int* comp_dc, const int* comp_ac) {
    select = 0;
    for (int c = 0; c < 3; ++c) select |= (uint32_t)(comp_dc[c] & 1) << c | (uint32_t)(comp_ac[c] & 1) << (4 + c);
  }
  JD_HD int dc(int comp) const { return (int)(select >> comp) & 1; }
  JD_HD int ac(int comp) const { return 2 + ((int)(select >> (4 + comp)) & 1); }
};

// one Huffman symbol: >= 0 and *len = its code length, or -1 = no code of this table (len = 16).  Bits behind the reader's last
// real bit read as zeros; the caller compares *len with r.cnt.
JD_HD int lookup(const Huff& h, Reader& r, int* len) {
  const uint32_t v = r.peek(16);
  const uint32_t e = h.fast[v >> 8];
  if (e) {
    const int l = (int)(e >> 8);
    *len = l < 1 ? 1 : (l > 8 ? 8 : l);                  // 1..8 whatever the table's bytes are: every symbol consumes a bit
    return (int)(e & 255u);
  }
  for (int l = 9; l <= 16; ++l) {
    if (v < h.limit[l]) {
      *len = l;
      return h.vals[(uint32_t)(h.offs[l] + (int)(v >> (16 - l))) & 255u];
    }
  }
  *len = 16;
  return -1;
}

// Decodes from state `st` until the position reaches end_bit (a subsequence's end) between two symbols, or the scan is over.
// WRITE = false: a synchronisation round.  Errors are noted in *err (the first one's RTV_JPEG_STATUS_* bit) and decoding goes on
// by a fixed rule, so that the exit state is a function of the entry state alone.  WRITE = true: the final pass from a settled
// state; coefficients go to `sink`, and the first error ends the decode.  Every loop below consumes at least one bit or one marker,
// so a call makes at most end_bit - st.bit + 1 steps.
template <bool WRITE, class Sink>
JD_HD State decode_subsequence(const Tables& T, const Geom& g, const uint8_t* scan, State st, uint32_t end_bit, Counts* counts, int* err,
                               Sink& sink) {
  Counts k = {0, 0};
  *err = 0;
  if (st.bit == END_BIT || st.bit >= end_bit) {
    *counts = k;
    return st;
  }
  Reader r;
  r.start(scan, (uint32_t)g.scan_bytes, st.bit);
  int zz = (int)(st.aux & 255u), slot = (int)(st.aux >> 8);
  bool ended = false;
  for (;;) {
    if (r.bound() >= end_bit && r.position() >= end_bit) break;
    const int comp = g.slot_comp(slot);
    const Huff& h = T.huff[zz == 0 ? T.dc(comp) : T.ac(comp)];
    int len, extra = 0;
    const int sym = lookup(h, r, &len);
    bool short_of_bits = len > r.cnt;                    // only a stopped reader can be short
    if (!short_of_bits && sym >= 0) {
      extra = zz == 0 ? sym : (sym & 15);
      if (zz == 0 && extra > 15) extra = 16;             // no DC size category: a bad code below
      if (extra <= 15) {
        if (r.cnt < len + extra) r.fill();
        short_of_bits = len + extra > r.cnt;
      }
    }
    if (short_of_bits) {                                 // the symbol runs into a marker or the end of the scan
      const int m = r.marker();
      if (m >= 0xD0 && m <= 0xD7 && g.ri > 0) {
        if (zz != 0 || slot != 0) {                      // a restart marker inside an MCU
          if (!*err) *err = RTV_JPEG_STATUS_MARKER;
          if (WRITE) {
            ended = true;
            break;
          }
        }
        if (WRITE) sink.at_marker(k);
        r.jump_marker();
        zz = 0, slot = 0;
        k = Counts{k.c + 1, 0};
        continue;
      }
      ended = true;                                      // EOI, another marker, or the end: the scan is over
      break;
    }
    if (sym < 0 || extra > 15) {
      if (!*err) *err = RTV_JPEG_STATUS_BAD_CODE;
      if (WRITE) {
        ended = true;
        break;
      }
      r.drop(len);                                       // a round goes on behind the pattern
      continue;
    }
    r.drop(len);
    int v = 0;
    if (extra) {
      v = (int)r.peek(extra);
      r.drop(extra);
      if (v < (1 << (extra - 1))) v -= (1 << extra) - 1;  // T.81 F.2.2.1 EXTEND
    }
    bool block_done = false;
    if (zz == 0) {
      if (WRITE) sink.put(k.c, k.n, slot, 0, v);           // the DC difference; the predictions are summed afterwards
      zz = 1;
    } else {
      const int run = sym >> 4;
      if (extra == 0) {
        if (run == 15) {                                 // ZRL
          zz += 16;
          block_done = zz > 63;
        } else {                                         // EOB (libjpeg reads every run with size 0 but 15 as one)
          block_done = true;
        }
      } else {
        zz += run;
        if (zz > 63) {
          if (!*err) *err = RTV_JPEG_STATUS_ZIGZAG;
          if (WRITE) {
            ended = true;
            break;
          }
          block_done = true;
        } else {
          if (WRITE) sink.put(k.c, k.n, slot, zz, v);
          ++zz;
          block_done = zz > 63;
        }
      }
    }
    if (block_done) {
      zz = 0;
      slot = slot + 1 == g.bpm ? 0 : slot + 1;
      ++k.n;
    }
  }
  *counts = k;
  State out;
  out.bit = ended ? END_BIT : r.position();
  out.aux = ended ? 0u : ((uint32_t)zz | ((uint32_t)slot << 8));
  return out;
}

// the state a round-0 decoder of subsequence i guesses: the start of an MCU, on a byte that is no stuffed one
JD_HD State guessed_state(const uint8_t* scan, uint32_t scan_bytes, uint32_t bit) {
  uint32_t p = bit >> 3;
  if (p > 0 && p < scan_bytes && scan[p] == 0x00 && scan[p - 1] == 0xFF) ++p;
  return State{p * 8u, 0u};
}

// ------------------------------------------------------------------------------------------------------------------ pixel stage
// libjpeg jidctint.c ("islow"), CONST_BITS = 13, PASS1_BITS = 2: one 8-point pass on in[0..7] (dequantised coefficients of a
// column, or a row of the first pass' results).  FIRST: out = DESCALE(., 11); else out = DESCALE(., 18), still to be range-limited.
template <bool FIRST>
JD_HD void idct8(const int* in, int* out) {
  const int SH = FIRST ? 11 : 18, RND = 1 << (SH - 1);
  int z2 = in[2], z3 = in[6];
  int z1 = (z2 + z3) * 4433;
  int tmp2 = z1 + z3 * -15137;
  int tmp3 = z1 + z2 * 6270;
  int tmp0 = (int)((unsigned)(in[0] + in[4]) << 13);
  int tmp1 = (int)((unsigned)(in[0] - in[4]) << 13);
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = in[7], tmp1 = in[5], tmp2 = in[3], tmp3 = in[1];
  z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2;
  int z4 = tmp1 + tmp3;
  const int z5 = (z3 + z4) * 9633;
  tmp0 *= 2446, tmp1 *= 16819, tmp2 *= 25172, tmp3 *= 12299;
  z1 *= -7373, z2 *= -20995, z3 *= -16069, z4 *= -3196;
  z3 += z5, z4 += z5;
  tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
  out[0] = (tmp10 + tmp3 + RND) >> SH;
  out[7] = (tmp10 - tmp3 + RND) >> SH;
  out[1] = (tmp11 + tmp2 + RND) >> SH;
  out[6] = (tmp11 - tmp2 + RND) >> SH;
  out[2] = (tmp12 + tmp1 + RND) >> SH;
  out[5] = (tmp12 - tmp1 + RND) >> SH;
  out[3] = (tmp13 + tmp0 + RND) >> SH;
  out[4] = (tmp13 - tmp0 + RND) >> SH;
}

// libjpeg's IDCT range limit: range_limit[x & 1023] of the table centred on 128
JD_HD int range_limit(int x) {
  x &= 1023;
  if (x < 512) return x + 128 > 255 ? 255 : x + 128;
  return x - 896 < 0 ? 0 : x - 896;
}

JD_HD int clamp255(int x) { return x < 0 ? 0 : (x > 255 ? 255 : x); }

// jdcolor.c, SCALEBITS = 16: the table values computed as they are built there
JD_HD void ycc_to_rgb(int y, int cb, int cr, uint8_t* rgb) {
  const int b = cb - 128, r = cr - 128;
  rgb[0] = (uint8_t)clamp255(y + ((91881 * r + 32768) >> 16));
  rgb[1] = (uint8_t)clamp255(y + ((-22554 * b + 32768 - 46802 * r) >> 16));
  rgb[2] = (uint8_t)clamp255(y + ((116130 * b + 32768) >> 16));
}

}  // namespace jd
}  // namespace rtv
