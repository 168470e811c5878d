// Driver of tests/test_fastq_parse_sanitized.py: a host program around the emulation build of the FASTQ parser (FQSX_EMU: the
// kernels of csrc/fqsx_fastq.h as 1-lane host "waves"), built with -fsanitize=address,undefined where the compiler can.  Every
// text lives in a heap buffer of exactly its size, and so do the emulated device buffers, so that a load or a store outside one
// ends the run.  The texts are the edge cases of tests/test_fastq_parse.py; every result is compared with a byte-by-byte
// splitter (four line feeds make a record).  Prints "DONE <texts> <records>".
#include "../../include/fqsx.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static int check(fqsx_fastq *h, const std::string &text, long &n_records) {
  std::vector<uint8_t> t(text.begin(), text.end());   // (exactly the text's bytes)
  uint64_t out[8];
  if (fqsx_fastq_index(h, t.empty() ? nullptr : t.data(), t.size(), out)) { printf("index: %s\n", fqsx_last_error()); return 1; }
  // the specification
  std::string ids, bases, quals;
  std::vector<uint64_t> id_off{0}, read_off{0}, qual_off{0};
  std::vector<uint32_t> plus;
  uint64_t consumed = 0, lfs = 0;
  {
    std::string f[4];
    int k = 0;
    for (size_t i = 0; i < t.size(); ++i) {
      if (t[i] != 0x0a) { f[k].push_back((char)t[i]); continue; }
      ++lfs;
      if (++k < 4) continue;
      ids += f[0] + "\n"; bases += f[1]; quals += f[3];
      id_off.push_back(ids.size()); read_off.push_back(bases.size()); qual_off.push_back(quals.size());
      plus.push_back((uint32_t)f[2].size());
      consumed = i + 1;
      for (auto &x : f) x.clear();
      k = 0;
    }
  }
  const uint64_t n = plus.size();
  if (out[0] != n || out[1] != consumed || out[2] != ids.size() || out[3] != bases.size() || out[4] != quals.size() || out[7] != lfs) {
    printf("summary differs for a text of %zu bytes\n", t.size());
    return 1;
  }
  std::vector<uint8_t> g_ids(out[2]), g_bases(out[3]), g_quals(out[4]);
  std::vector<uint64_t> g_io(n + 1), g_ro(n + 1), g_qo(n + 1);
  std::vector<uint32_t> g_plus(n);
  if (fqsx_fastq_columns(h, g_ids.data(), g_io.data(), g_bases.data(), g_ro.data(), g_quals.data(), g_qo.data(), g_plus.data())) {
    printf("columns: %s\n", fqsx_last_error());
    return 1;
  }
  auto differ = [](const std::vector<uint8_t> &v, const std::string &s) { return v.size() != s.size() || !std::equal(v.begin(), v.end(), s.begin(), [](uint8_t a, char b) { return a == (uint8_t)b; }); };
  if (differ(g_ids, ids) || differ(g_bases, bases) || differ(g_quals, quals) ||
      g_io != id_off || g_ro != read_off || g_qo != qual_off || g_plus != plus) {
    printf("columns differ for a text of %zu bytes\n", t.size());
    return 1;
  }
  n_records += (long)n;
  return 0;
}

int main() {
  fqsx_fastq *h = nullptr;
  if (fqsx_fastq_create(0, 0, &h)) { printf("create: %s\n", fqsx_last_error()); return 1; }
  std::vector<std::string> texts = {"", "no line feed", "\n", "\n\n\n", "\n\n\n\n", "\n\n\n\n\n", std::string(4099, '\n'),
                                    "@\nAC\n+\n!!\n@e\n\n+\n\n\n\n\n\n@x\r\nAC\r\n+x\r\n!!\r\n@partial\nACG"};
  // records around the 16 KiB tile boundary: a line feed as the last byte of a tile and as the first of the next, a line longer
  // than a tile, and every residue of the length mod 16
  std::string big;
  for (int i = 0; big.size() < 16384 - 200; ++i) big += "@r." + std::to_string(i) + "\n" + std::string(30 + i % 70, "ACGTN"[i % 5]) + "\n+\n" + std::string(30 + i % 70, '5') + "\n";
  big += "@" + std::string(16384 - 2 - big.size(), 'p') + "\n\n+\n\n";
  big += "@long\n" + std::string(40000, 'A') + "\n+long\n" + std::string(40000, '#') + "\n@tail\nAC\n+\n!!\n";
  if (big[16383] != '\n' || big[16384] != '\n') { printf("the boundary text is not what it should be\n"); return 1; }
  for (size_t n : {(size_t)16383, (size_t)16384, (size_t)16385, big.size()}) texts.push_back(big.substr(0, n));
  for (size_t k = 0; k < 16; ++k) texts.push_back(big.substr(0, 16384 + 3000 + k));
  long n_records = 0;
  for (const auto &t : texts)
    if (check(h, t, n_records)) return 1;
  fqsx_fastq_destroy(h);
  printf("DONE %zu %ld\n", texts.size(), n_records);
  return 0;
}
