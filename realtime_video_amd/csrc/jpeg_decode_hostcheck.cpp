// Stand-alone host program over jpeg_decode_core.h, not linked into the library (make hostcheck; make hostcheck SANITIZE=1 builds
// it with -fsanitize=address,undefined).  It emulates the entropy kernel of jpeg_decode.hip serially - the same rounds over the
// same subsequences with the same state machine, then the block count scan, the final pass and the DC sums - so that
//   * the scheme can be compared with a serial decoder on the CPU, at any subsequence length, and
//   * damaged files meet the bounds checks here, under the sanitizers, before they meet them on a GPU.
//
//   jpeg_decode_hostcheck SUBSEQ_BITS OUT_DIR FILE...
// prints one line per file, "<file> status <word> rounds <r> subsequences <n>" or "<file> refused <reason>", and writes the
// coefficients (int16, the layout of rtv_jpeg_decode_coefficients) to OUT_DIR/<basename>.coef.  Exit status 0 unless a file
// cannot be read or written.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "jpeg_decode_core.h"

using namespace rtv;

static int decode_file(const char* path, int subseq_bits, const char* out_dir) {
  FILE* fp = fopen(path, "rb");
  if (!fp) return fprintf(stderr, "cannot open %s\n", path), 1;
  std::vector<uint8_t> file;
  uint8_t buf[65536];
  for (size_t n; (n = fread(buf, 1, sizeof(buf), fp)) > 0;) file.insert(file.end(), buf, buf + n);
  fclose(fp);
  // an exactly-sized heap copy: a read past the file's last byte is a heap overflow the sanitizer reports
  std::vector<uint8_t> exact(file.begin(), file.end());
  rtv_jpeg_desc desc;
  jd::Geom g;
  const char* why = jd::parse(exact.data(), exact.size(), &desc);
  if (!why) why = jd::geom_from_desc(desc, &g);
  if (why) {
    printf("%s refused %s\n", path, why);
    return 0;
  }
  static const uint8_t natural[64] = JD_NATURAL_ORDER;
  jd::Tables T;
  T.huff = (const jd::Huff*)desc.huff, T.natural = natural;
  T.set(desc.comp_dc, desc.comp_ac);
  // the scan in a heap block of its own size, for the same reason
  std::vector<uint8_t> scanv(exact.begin() + g.scan_offset, exact.begin() + g.scan_offset + g.scan_bytes);
  const uint8_t* scan = scanv.data();
  std::vector<int16_t> coef((size_t)g.coef_elems(), 0);

  const uint32_t L = (uint32_t)jd::effective_subseq_bits(subseq_bits, g.scan_bytes);
  const uint32_t nbits = (uint32_t)g.scan_bytes * 8u;
  const int nsub = nbits ? (int)((nbits + L - 1) / L) : 1;
  if (nsub > jd::MAX_SUBSEQ) return fprintf(stderr, "%s: %d subsequences\n", path, nsub), 1;
  std::vector<jd::State> entry(nsub), exits(nsub);
  std::vector<jd::Counts> cnt(nsub);
  std::vector<int> err(nsub);
  auto end_bit = [&](int i) { return i == nsub - 1 ? jd::END_BIT - 1u : (uint32_t)(i + 1) * L; };
  jd::NullSink none;
  for (int i = 0; i < nsub; ++i) {
    entry[i] = i == 0 ? jd::State{0u, 0u} : jd::guessed_state(scan, (uint32_t)g.scan_bytes, (uint32_t)i * L);
    exits[i] = jd::decode_subsequence<false>(T, g, scan, entry[i], end_bit(i), &cnt[i], &err[i], none);
  }
  int round = 1;
  for (; round <= nsub; ++round) {
    std::vector<jd::State> want(entry);
    for (int i = 1; i < nsub; ++i) want[i] = exits[i - 1];
    bool any = false;
    for (int i = 0; i < nsub; ++i) {
      if (want[i] == entry[i]) continue;
      any = true;
      entry[i] = want[i];
    }
    if (!any) break;
    for (int i = 0; i < nsub; ++i)                       // (a thread whose entry state is unchanged would compute the same again)
      exits[i] = jd::decode_subsequence<false>(T, g, scan, entry[i], end_bit(i), &cnt[i], &err[i], none);
  }
  int first_err = jd::MAX_SUBSEQ;
  for (int i = nsub - 1; i >= 0; --i)
    if (err[i]) first_err = i;
  jd::Counts base = {0, 0};
  int status = 0, reached = 0;
  for (int i = 0; i < nsub; ++i) {
    if (i <= first_err) {
      jd::CoefSink sink = {coef.data(), natural, g, base, 0, 0};
      jd::Counts again;
      int e;
      jd::decode_subsequence<true>(T, g, scan, entry[i], end_bit(i), &again, &e, sink);
      status |= sink.status | e;
      reached = sink.reached > reached ? sink.reached : reached;
    }
    base = jd::combine(base, cnt[i]);
  }
  const long long done = (long long)base.c * g.ri * g.bpm + base.n;
  if (first_err == jd::MAX_SUBSEQ && done < g.total_blocks()) status |= RTV_JPEG_STATUS_SHORT;
  for (int c = 0; c < g.ncomp; ++c) {
    const int slot0 = c ? g.hs * g.vs + c - 1 : 0, slots = c ? 1 : g.hs * g.vs;
    int pred = 0;
    for (int m = 0; m < g.mcu_cols * g.mcu_rows; ++m) {
      if (g.ri > 0 && m % g.ri == 0) pred = 0;
      for (int s = slot0; s < slot0 + slots; ++s) {
        if (m * g.bpm + s >= reached) continue;
        int16_t* p = coef.data() + g.block_offset(m, s);
        pred += *p;
        *p = (int16_t)pred;
      }
    }
  }
  printf("%s status %d rounds %d subsequences %d\n", path, status, round, nsub);
  std::string name(path);
  const size_t slash = name.find_last_of('/');
  const std::string out = std::string(out_dir) + "/" + (slash == std::string::npos ? name : name.substr(slash + 1)) + ".coef";
  FILE* fo = fopen(out.c_str(), "wb");
  if (!fo) return fprintf(stderr, "cannot write %s\n", out.c_str()), 1;
  fwrite(coef.data(), sizeof(int16_t), coef.size(), fo);
  fclose(fo);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 4) return fprintf(stderr, "usage: %s SUBSEQ_BITS OUT_DIR FILE...\n", argv[0]), 2;
  const int subseq_bits = atoi(argv[1]);
  if (subseq_bits < 0 || (subseq_bits && (subseq_bits < 32 || subseq_bits % 32))) return fprintf(stderr, "bad SUBSEQ_BITS\n"), 2;
  for (int i = 3; i < argc; ++i)
    if (decode_file(argv[i], subseq_bits, argv[2])) return 1;
  return 0;
}
