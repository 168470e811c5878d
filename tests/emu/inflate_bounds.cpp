// inflate_bounds.cpp -- the inflate kernel's bounds on damaged members, for a host build under the sanitizers.
//
// A stand-alone program around the 1-lane emulation of k_bgzf_inflate (csrc/fqsx_inflate.h).  It reads a BGZF file, and gives
// the kernel every member three ways: as it is; cut short after every k-th byte of its deflate data; and with every k-th bit of
// its deflate data and trailer flipped.  Each run gets the member in a heap block of exactly its size and a text buffer of
// exactly the ISIZE the (possibly damaged) trailer states, so that AddressSanitizer sees any byte read outside the member and
// any byte written outside its text; the status word must be a known kind, and an undamaged member must come out as the file
// says.  Nothing here runs on a GPU or inside Python:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -DFQSX_EMU -x c++ tests/emu/inflate_bounds.cpp \
//       fqsqueezer_amd/csrc/fqsx_host.cpp -o inflate_bounds && ./inflate_bounds file.bgzf [k]
#include "../../fqsqueezer_amd/csrc/fqsx_inflate.h"
#include "../../include/fqsx.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static u64 g_runs = 0, g_kinds[INF_N_KINDS];

// one member (n bytes) through the kernel; returns its status, the text in `text`
static u32 run(const u8 *m, u64 n, std::vector<u8> &text) {
  u8 *in = (u8 *)malloc(n ? n : 1);
  memcpy(in, m, n);
  u32 isize = n >= 4 ? (u32)in[n - 4] | ((u32)in[n - 3] << 8) | ((u32)in[n - 2] << 16) | ((u32)in[n - 1] << 24) : 0;
  if (isize > INF_WINDOW) isize = INF_WINDOW + 1;   // (the host refuses such a member before the launch: the kernel has to as well)
  const u64 shift = g_runs % 16;                    // the text at every alignment
  u8 *out = (u8 *)malloc(shift + isize + 1);
  u64 in_off[2] = {0, n}, out_off[2] = {0, isize};
  u32 status = ~0u;
  InfCfg c;
  c.in = in; c.in_off = in_off; c.out = out + shift; c.out_off = out_off; c.out_cap = isize; c.status = &status; c.n = 1;
  fq_emu_block = 0;
  fq_emu_nblocks = 1;
  k_bgzf_inflate(c);
  if (status >= INF_N_KINDS) { fprintf(stderr, "status %u is no kind\n", status); exit(1); }
  g_runs += 1;
  g_kinds[status] += 1;
  text.assign(out + shift, out + shift + (status == INF_OK ? isize : 0));
  free(out);
  free(in);
  return status;
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: inflate_bounds file.bgzf [every k-th bit, default 1]\n"); return 2; }
  const u64 step = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<u8> file;
  u8 buf[1 << 16];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) file.insert(file.end(), buf, buf + k);
  fclose(f);
  std::vector<u64> off(file.size() / 28 + 1);
  std::vector<u32> isize(off.size());
  u64 sc[4];
  if (fqsx_bgzf_scan(file.data(), file.size(), (u32)off.size(), off.data(), isize.data(), sc) || sc[2] || sc[3]) {
    fprintf(stderr, "%s is not a whole BGZF file\n", argv[1]);
    return 2;
  }
  std::vector<u8> text, t2;
  for (u64 i = 0; i < sc[0]; ++i) {
    const u8 *m = file.data() + off[i];
    const u64 n = (i + 1 < sc[0] ? off[i + 1] : sc[1]) - off[i];
    if (run(m, n, text) != INF_OK || text.size() != isize[i]) { fprintf(stderr, "member %llu does not inflate\n", (unsigned long long)i); return 1; }
    const u64 data = 12 + ((u64)m[10] | ((u64)m[11] << 8));
    std::vector<u8> d(m, m + n);
    for (u64 cut = data; cut + 8 < n; cut += step) {   // the deflate data cut short, the trailer behind it
      std::vector<u8> s(m, m + cut);
      s.insert(s.end(), m + n - 8, m + n);
      if (run(s.data(), s.size(), t2) == INF_OK && t2 != text) { fprintf(stderr, "member %llu cut at %llu: accepted with another text\n", (unsigned long long)i, (unsigned long long)cut); return 1; }
    }
    for (u64 bit = 8 * data; bit < 8 * n; bit += step) {
      d[bit >> 3] ^= (u8)(1u << (bit & 7));
      if (run(d.data(), n, t2) == INF_OK && t2 != text) { fprintf(stderr, "member %llu bit %llu: accepted with another text\n", (unsigned long long)i, (unsigned long long)bit); return 1; }
      d[bit >> 3] ^= (u8)(1u << (bit & 7));
    }
    for (u64 cut = 0; cut < data + 8 && cut < n; ++cut) run(m, cut, t2);   // no room for a header and a trailer
  }
  printf("%llu members, %llu runs:", (unsigned long long)sc[0], (unsigned long long)g_runs);
  for (u32 k = 0; k < INF_N_KINDS; ++k) printf(" kind %u x %llu", k, (unsigned long long)g_kinds[k]);
  printf("\n");
  return 0;
}
