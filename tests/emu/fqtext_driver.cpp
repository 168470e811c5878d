// Driver of tests/test_fastq_text_sanitized.py: a host program around the emulation build of the text assembler (FQSX_EMU:
// the kernels of csrc/fqsx_fqtext.h as 1-lane host "waves"), built with -fsanitize=address,undefined where the compiler can.
// Every column lives in a heap buffer of exactly its size, so that a load outside one ends the run; every text is compared
// with a record-by-record loop.  The cases are those of tests/test_fastq_text.py: lengths and alignments, record counts at
// the lane, wave and tile edges, constant ids and fill-byte qualities, refused calls.  Prints "DONE <cases> <records>".
#include "../../include/fqsx.h"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

struct Block {
  std::vector<std::string> ids, seqs, quals;
};

static uint32_t rnd(uint64_t &s) {
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(s >> 33);
}

static void add(Block &b, uint32_t L, uint32_t il, uint64_t &s) {
  std::string id, seq, q;
  for (uint32_t k = 0; k + 1 < il; ++k) id.push_back(k ? (char)('0' + rnd(s) % 70) : '@');
  id.push_back('\n');
  for (uint32_t k = 0; k < L; ++k) { seq.push_back("ACGTN"[rnd(s) % 5]); q.push_back((char)(33 + rnd(s) % 41)); }
  b.ids.push_back(id); b.seqs.push_back(seq); b.quals.push_back(q);
}

// what the block must come out as; no_ids / no_quals: the constant id line, the fill byte
static void expect(const Block &b, int paired, bool no_ids, bool no_quals, int fill, std::string out[2]) {
  out[0].clear(); out[1].clear();
  for (size_t i = 0; i < b.ids.size(); ++i)
    out[paired ? i & 1 : 0] += (no_ids ? std::string("@\n") : b.ids[i]) + b.seqs[i] + "\n+\n" + (no_quals ? std::string(b.seqs[i].size(), (char)fill) : b.quals[i]) + "\n";
}

struct Columns {
  std::vector<uint8_t> ids, bases, quals;   // (exactly their bytes)
  std::vector<uint32_t> id_len;
  std::vector<uint64_t> read_off;
};
static Columns columns(const Block &b) {
  Columns c;
  c.read_off.push_back(0);
  for (size_t i = 0; i < b.ids.size(); ++i) {
    c.ids.insert(c.ids.end(), b.ids[i].begin(), b.ids[i].end());
    c.bases.insert(c.bases.end(), b.seqs[i].begin(), b.seqs[i].end());
    c.quals.insert(c.quals.end(), b.quals[i].begin(), b.quals[i].end());
    c.id_len.push_back((uint32_t)b.ids[i].size());
    c.read_off.push_back(c.bases.size());
  }
  c.ids.shrink_to_fit(); c.bases.shrink_to_fit(); c.quals.shrink_to_fit(); c.id_len.shrink_to_fit();
  return c;
}

static int text_is(fqsx_fqtext *h, const uint64_t nb[2], const std::string want[2], const char *what) {
  for (int m = 0; m < 2; ++m) {
    if (nb[m] != want[m].size()) { printf("%s: output %d has %llu bytes, not %zu\n", what, m, (unsigned long long)nb[m], want[m].size()); return 1; }
    std::vector<uint8_t> got(nb[m]);
    if (fqsx_fqtext_download(h, m, got.empty() ? nullptr : got.data())) { printf("%s: download: %s\n", what, fqsx_last_error()); return 1; }
    if (nb[m] && memcmp(got.data(), want[m].data(), nb[m])) { printf("%s: output %d differs\n", what, m); return 1; }
  }
  return 0;
}

// ids_on_device 1: in the emulation the columns are "device memory" as they are; 0: the call copies them first
static int run(fqsx_fqtext *h, const Block &b, int paired, bool no_ids, bool no_quals, int on_device, const char *what, long &n_records) {
  const Columns c = columns(b);
  const int fill = 33 + 7;
  std::string want[2];
  expect(b, paired, no_ids, no_quals, fill, want);
  uint64_t nb[2] = {~0ull, ~0ull};
  const int rc = fqsx_fqtext_block(h, (uint32_t)b.ids.size(), paired, no_ids ? nullptr : c.ids.data(), no_ids ? nullptr : c.id_len.data(), on_device,
                                   no_ids ? 0 : c.ids.size(), c.bases.data(), no_quals ? nullptr : c.quals.data(), fill, c.read_off.data(), nb);
  if (rc) { printf("%s: %d: %s\n", what, rc, fqsx_last_error()); return 1; }
  n_records += (long)b.ids.size();
  return text_is(h, nb, want, what);
}

int main() {
  fqsx_fqtext *h = nullptr;
  if (fqsx_fqtext_create(0, &h)) { printf("create: %s\n", fqsx_last_error()); return 1; }
  uint64_t s = 12345;
  long n_cases = 0, n_records = 0;
  // 1. lengths and alignments
  {
    const uint32_t Ls[] = {0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 150, 151}, ils[] = {1, 2, 3, 17, 64, 65};
    Block b;
    for (int rep = 0; rep < 8; ++rep)
      for (int k = 0; k < 84; ++k) {
        const int j = (k + 5 * rep) % 84;
        add(b, Ls[j / 6], ils[j % 6], s);
      }
    for (int paired = 0; paired < 2; ++paired)
      for (int on_device = 0; on_device < 2; ++on_device, ++n_cases)
        if (run(h, b, paired, false, false, on_device, "alignments", n_records)) return 1;
  }
  // 2. record counts
  for (uint32_t n : {0u, 1u, 2u, 3u, 63u, 64u, 65u, 2047u, 2048u, 2049u, 4097u})
    for (int paired = 0; paired < 2; ++paired, ++n_cases) {
      Block b;
      for (uint32_t i = 0; i < n + (paired ? n & 1 : 0); ++i) add(b, rnd(s) % 41, 1 + rnd(s) % 20, s);
      if (run(h, b, paired, false, false, 1, "counts", n_records)) return 1;
    }
  // 5. constant ids, fill-byte qualities
  for (int which = 1; which < 4; ++which)
    for (int paired = 0; paired < 2; ++paired, ++n_cases) {
      Block b;
      for (uint32_t i = 0; i < 300; ++i) add(b, rnd(s) % 71, 1 + rnd(s) % 20, s);
      if (run(h, b, paired, (which & 1) != 0, (which & 2) != 0, 1, "constants", n_records)) return 1;
    }
  // 8. refused calls: each leaves the text of the block before it, and the handle works afterwards
  for (int what = 0; what < 4; ++what, ++n_cases) {
    Block first, bad, after;
    for (uint32_t i = 0; i < 700; ++i) add(first, rnd(s) % 41, 1 + rnd(s) % 20, s);
    for (uint32_t i = 0; i < 301; ++i) add(bad, 1 + rnd(s) % 40, 1 + rnd(s) % 20, s);
    for (uint32_t i = 0; i < 64; ++i) add(after, rnd(s) % 41, 1 + rnd(s) % 20, s);
    if (run(h, first, 1, false, false, 1, "before a refused call", n_records)) return 1;
    std::string before[2];
    expect(first, 1, false, false, 0, before);
    const uint64_t nb_before[2] = {before[0].size(), before[1].size()};
    Columns c = columns(bad);
    int paired = 0;
    if (what == 0) c.read_off[150] = c.read_off[149] - 1;                                             // offsets that descend
    if (what == 1) { c.id_len[8] += c.id_len[7]; c.id_len[7] = 0; }                                   // an id line of 0 bytes
    if (what == 2) { c.ids.insert(c.ids.end(), 8, (uint8_t)'x'); c.ids.shrink_to_fit(); }             // lengths that do not add up to id_bytes
    if (what == 3) paired = 1;                                                                        // paired, 301 reads
    uint64_t nb[2] = {0, 0};
    const int rc = fqsx_fqtext_block(h, 301, paired, c.ids.data(), c.id_len.data(), 1, c.ids.size(), c.bases.data(), c.quals.data(), 0, c.read_off.data(), nb);
    if (rc != FQSX_E_ARG) { printf("refused call %d returned %d\n", what, rc); return 1; }
    if (text_is(h, nb_before, before, "after a refused call")) return 1;
    if (run(h, after, 0, false, false, 0, "after a refused call", n_records)) return 1;
  }
  fqsx_fqtext_destroy(h);
  printf("DONE %ld %ld\n", n_cases, n_records);
  return 0;
}
