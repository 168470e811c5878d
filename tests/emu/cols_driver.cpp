// Driver of tests/test_device_columns_sanitized.py: a host program around the emulation build of the device-resident columns
// (FQSX_EMU: the kernels of csrc/fqsx_cols.h and csrc/fqsx_fastq.h as 1-lane host "waves"), built with
// -fsanitize=address,undefined where the compiler can.  The emulated device buffers are heap buffers, so a load or a store
// outside one ends the run.  Stores are filled chunk by chunk from edge texts (empty reads, read lengths around 16 and 64, a read
// longer than a parser tile), blocks are cut single-end and paired in several orders and compared with a byte-by-byte splitter,
// and every refusal is checked to leave the store and the previous block as they were.  Prints "DONE <gathers> <refusals>".
#include "../../include/fqsx.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

struct Spec { std::vector<std::string> bases, quals; };   // the records of a store, as the specification splits the texts

static int fail(const char *what) { printf("%s: %s\n", what, fqsx_last_error()); return 1; }

// the text of n records (lengths from `lens`, cyclically from `first`), appended to the store as one chunk and to its specification
static int append(fqsx_fastq *p, fqsx_cols *s, Spec &spec, const std::vector<size_t> &lens, size_t first, size_t n, const char *tail) {
  std::string text;
  for (size_t i = 0; i < n; ++i) {
    const size_t k = lens[(first + i) % lens.size()];
    std::string b(k, 'A'), q(k, '!');
    for (size_t j = 0; j < k; ++j) { b[j] = "ACGTN"[(i + 3 * j + first) % 5]; q[j] = (char)(33 + (7 * i + j + first) % 41); }
    text += "@r" + std::to_string(spec.bases.size()) + "\n" + b + "\n+\n" + q + "\n";
    spec.bases.push_back(b); spec.quals.push_back(q);
  }
  text += tail;   // (a partial record behind the last complete one: not consumed)
  std::vector<uint8_t> t(text.begin(), text.end());
  uint64_t out[8];
  if (fqsx_fastq_index(p, t.empty() ? nullptr : t.data(), t.size(), out)) return fail("index");
  if (out[0] != n) { printf("records differ\n"); return 1; }
  std::vector<uint8_t> ids(out[2]);
  std::vector<uint64_t> id_off(n + 1), read_off(n + 1);
  std::vector<uint32_t> plus(n);
  if (fqsx_fastq_columns_into(p, s, ids.data(), id_off.data(), read_off.data(), plus.data())) return fail("columns_into");
  uint64_t at = 0;
  for (size_t i = 0; i < n; ++i) {
    if (read_off[i] != at || plus[i] != 1) { printf("host arrays of the chunk differ\n"); return 1; }
    at += spec.bases[spec.bases.size() - n + i].size();
  }
  if (read_off[n] != at || id_off[n] != ids.size()) { printf("host arrays of the chunk differ\n"); return 1; }
  return 0;
}

struct Block { std::vector<uint8_t> bases, quals; std::vector<uint64_t> off; };

static Block expected(const Spec &a, const Spec *b, const std::vector<uint32_t> &idx) {
  Block k;
  k.off.push_back(0);
  for (uint32_t r : idx)
    for (const Spec *s : {&a, b}) {
      if (!s) continue;
      k.bases.insert(k.bases.end(), s->bases[r].begin(), s->bases[r].end());
      k.quals.insert(k.quals.end(), s->quals[r].begin(), s->quals[r].end());
      k.off.push_back(k.bases.size());
    }
  return k;
}

static int download(fqsx_cols *s, const uint8_t *d_bases, const uint8_t *d_quals, const uint64_t *d_off, size_t n_off, Block &k) {
  k.off.assign(n_off, 0);
  if (fqsx_cols_download(s, d_off, k.off.data(), n_off * sizeof(uint64_t))) return fail("download");
  k.bases.assign(k.off.back(), 0); k.quals.assign(k.off.back(), 0);
  if (fqsx_cols_download(s, d_bases, k.bases.data(), k.bases.size()) || fqsx_cols_download(s, d_quals, k.quals.data(), k.quals.size())) return fail("download");
  return 0;
}

static long n_gathers = 0, n_refusals = 0;
static const uint8_t *g_bases, *g_quals;
static const uint64_t *g_off;

static int gather(fqsx_cols *a, const Spec &sa, fqsx_cols *b, const Spec *sb, const std::vector<uint32_t> &idx) {
  const Block want = expected(sa, sb, idx);
  if (fqsx_cols_gather(a, b, idx.empty() ? nullptr : idx.data(), (uint32_t)idx.size(), want.off.data(), &g_bases, &g_quals, &g_off)) return fail("gather");
  Block got;
  if (download(a, g_bases, g_quals, g_off, want.off.size(), got)) return 1;
  if (got.bases != want.bases || got.quals != want.quals || got.off != want.off) { printf("a block of %zu reads differs\n", want.off.size() - 1); return 1; }
  ++n_gathers;
  return 0;
}

// a call that has to fail with `code` and leave the block gathered last (want) where it is
static int refused(fqsx_cols *a, fqsx_cols *b, const std::vector<uint32_t> &idx, const std::vector<uint64_t> &off, int code, const Block &want) {
  const uint8_t *x = nullptr, *y = nullptr;
  const uint64_t *z = nullptr;
  const int rc = fqsx_cols_gather(a, b, idx.data(), (uint32_t)idx.size(), off.data(), &x, &y, &z);
  if (rc != code) { printf("a gather that had to be refused with %d returned %d\n", code, rc); return 1; }
  Block got;
  if (download(a, g_bases, g_quals, g_off, want.off.size(), got)) return 1;
  if (got.bases != want.bases || got.quals != want.quals || got.off != want.off) { printf("a refused gather changed the previous block\n"); return 1; }
  ++n_refusals;
  return 0;
}

int main() {
  fqsx_fastq *p = nullptr;
  fqsx_cols *a = nullptr, *b = nullptr, *e = nullptr;
  if (fqsx_fastq_create(0, 0, &p) || fqsx_cols_create(0, &a) || fqsx_cols_create(0, &b) || fqsx_cols_create(0, &e)) return fail("create");
  const std::vector<size_t> la = {0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 31, 33}, lb = {64, 0, 257, 1, 16, 15, 17, 256, 65, 63, 255};
  Spec sa, sb;
  // four chunks each (the second of them a single record longer than a 16 KiB parser tile), 700 records in all
  const size_t parts[4] = {300, 1, 130, 269};
  for (int k = 0; k < 4; ++k) {
    const std::vector<size_t> one = {40000};
    if (append(p, a, sa, k == 1 ? one : la, 5 * k, parts[k], k % 2 ? "@partial\nAC" : "")) return 1;
    if (append(p, b, sb, k == 1 ? one : lb, 3 * k, parts[k], "")) return 1;
  }
  uint64_t info[4], info_b[4];
  if (fqsx_cols_info(a, info) || info[0] != 700 || info[3] != info[2]) { printf("info differs\n"); return 1; }
  // an index array of n reads: identity, reversed, strided across the chunks, one index repeated
  for (size_t n : {(size_t)0, (size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)255, (size_t)256, (size_t)257, (size_t)700})
    for (int pattern = 0; pattern < 4; ++pattern) {
      std::vector<uint32_t> idx(n);
      for (size_t i = 0; i < n; ++i) idx[i] = (uint32_t)(pattern == 0 ? i : pattern == 1 ? 699 - i : pattern == 2 ? (i * 271) % 700 : (i % 3 ? (i * 89) % 700 : 300));
      if (gather(a, sa, nullptr, nullptr, idx) || gather(a, sa, b, &sb, idx) || gather(b, sb, a, &sa, idx)) return 1;
    }
  // refusals, single-end and paired, behind a block of 90 reads / pairs
  for (int paired = 0; paired < 2; ++paired) {
    std::vector<uint32_t> idx(90);
    for (size_t i = 0; i < idx.size(); ++i) idx[i] = (uint32_t)((i * 271 + 5) % 700);
    if (gather(a, sa, paired ? b : nullptr, paired ? &sb : nullptr, idx)) return 1;
    const Block want = expected(sa, paired ? &sb : nullptr, idx);
    std::vector<uint32_t> bad = idx;
    bad[44] = 700;                       // one past the last record
    if (refused(a, paired ? b : nullptr, bad, want.off, FQSX_E_ARG, want)) return 1;
    bad[44] = 0xffffffffu;
    if (refused(a, paired ? b : nullptr, bad, want.off, FQSX_E_ARG, want)) return 1;
    for (size_t k : {(size_t)1, (size_t)37, want.off.size() - 1})
      for (int d = -1; d <= 1; d += 2) {
        std::vector<uint64_t> off = want.off;
        if (d < 0 && off[k] == off[k - 1]) continue;   // (an empty read cannot be a byte shorter)
        off[k] += (uint64_t)(int64_t)d;
        if (refused(a, paired ? b : nullptr, idx, off, FQSX_E_ARG, want)) return 1;
      }
    std::vector<uint64_t> off = want.off;
    off[0] = 1;                          // offsets that do not start at 0
    if (refused(a, paired ? b : nullptr, idx, off, FQSX_E_ARG, want)) return 1;
    if (gather(a, sa, paired ? b : nullptr, paired ? &sb : nullptr, idx)) return 1;
  }
  // an empty store: the empty block, then every index is refused
  {
    Spec none;
    if (gather(e, none, nullptr, nullptr, {})) return 1;
    const Block want = expected(none, nullptr, {});
    if (refused(e, nullptr, {0, 0, 0}, {0, 0, 0, 0}, FQSX_E_ARG, want)) return 1;
    if (refused(e, nullptr, {0}, {0, 5}, FQSX_E_ARG, want)) return 1;
  }
  // a chunk with a mismatched quality line is not appended
  {
    const std::string text = "@x\nACGT\n+\n!!!!\n@y\nACGT\n+\n!!!\n";
    uint64_t out[8];
    if (fqsx_fastq_index(p, (const uint8_t *)text.data(), text.size(), out) || out[0] != 2 || out[6] != 1) return fail("index of the mismatched chunk");
    std::vector<uint8_t> ids(out[2]);
    std::vector<uint64_t> id_off(3), read_off(3);
    std::vector<uint32_t> plus(2);
    if (fqsx_fastq_columns_into(p, b, ids.data(), id_off.data(), read_off.data(), plus.data()) != FQSX_E_ARG) { printf("a mismatched chunk was appended\n"); return 1; }
    if (fqsx_cols_info(b, info_b) || info_b[0] != 700 || info_b[3] != info_b[2]) { printf("a refused chunk changed the store\n"); return 1; }
    ++n_refusals;
    if (append(p, b, sb, lb, 1, 20, "")) return 1;
    std::vector<uint32_t> idx = {719, 0, 700, 300, 699};
    if (gather(b, sb, nullptr, nullptr, idx)) return 1;
  }
  // the whole base column
  {
    std::string want;
    for (const auto &x : sa.bases) want += x;
    std::vector<uint8_t> got(want.size());
    if (fqsx_cols_bases(a, got.data())) return fail("bases");
    if (!std::equal(got.begin(), got.end(), want.begin(), [](uint8_t u, char c) { return u == (uint8_t)c; })) { printf("the base column differs\n"); return 1; }
  }
  fqsx_cols_destroy(a);
  fqsx_cols_destroy(b);
  fqsx_cols_destroy(e);
  fqsx_fastq_destroy(p);
  printf("DONE %ld %ld\n", n_gathers, n_refusals);
  return 0;
}
