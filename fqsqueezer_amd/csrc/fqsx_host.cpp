// fqsx_host.cpp -- host-side (CPU) plumbing that travels with the DNA path: the read-length
// ("meta") stream every .fqs block carries (reference fqs/meta.cpp:31-73, application.cpp:633), the read-id
// stream (fqs/id.cpp, SURVEY.md §8f row N4: string tokeniser + delta coder; the host twin of the GPU coder csrc/fqsx_idk.h,
// which the tests compare it with byte for byte) and the
// per-bin read order of sorted mode.  None of it is on the hot path; it exists so that a complete container
// can be written around the GPU DNA / quality streams and handed to the reference decoder.
#include "../../include/fqsx.h"
#include "fqsx_split.h"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

namespace {
typedef uint64_t u64;
typedef uint32_t u32;
typedef uint8_t u8;

struct Enc {  // CRangeEncoder, sub_rc.h:32-87
  u64 low, range;
  std::vector<u8> out;
  void start() { low = 0; range = 0xff00000000000000ULL; out.clear(); }
  void encode(u64 f, u64 c, u64 t) {
    const u64 Top = 0x00ffffffffffffULL, M = 0xff00000000000000ULL;
    range /= t; low += range * c; range *= f;
    while (range <= Top) {
      if ((low ^ (low + range)) & M) range = (low | Top) - low;
      out.push_back((u8)(low >> 56));
      low <<= 8; range <<= 8;
    }
  }
  void end() { for (int i = 0; i < 8; ++i) { out.push_back((u8)(low >> 56)); low <<= 8; } }
};
struct Dec {  // CRangeDecoder, sub_rc.h:93-158, on a buffer of n bytes; `over`: bytes asked for beyond its end (they read as 0)
  u64 low, range, buf;
  const u8 *p;
  u64 n, pos, over;
  u64 byte() { if (pos < n) return p[pos++]; ++over; return 0; }
  void start(const u8 *p_, u64 n_) {
    p = p_; n = n_; pos = 0; over = 0; buf = 0;
    for (int i = 1; i <= 8; ++i) buf |= byte() << (64 - i * 8);
    low = 0; range = 0xff00000000000000ULL;
  }
  u64 cum(u64 t) { range /= t; return buf / range; }
  void update(u64 f, u64 c) {
    const u64 Top = 0x00ffffffffffffULL, M = 0xff00000000000000ULL;
    const u64 r = c * range;
    buf -= r; low += r; range *= f;
    while (range <= Top) {
      if ((low ^ (low + range)) & M) range = (low | Top) - low;
      buf = (buf << 8) + byte();
      low <<= 8; range <<= 8;
    }
  }
};
struct Model256 {  // CRangeCoderModel(256 symbols, adder 1, max_total 1<<15), meta.cpp:33-38, rc.h:344-405
  u32 st[256], total;
  Model256() { for (auto &x : st) x = 1; total = 256; }
  void encode(Enc &e, u32 x) {
    u32 cum = 0;
    for (u32 i = 0; i < x; ++i) cum += st[i];
    e.encode(st[x], cum, total);
    st[x] += 1; total += 1;
    while (total >= (1u << 15)) { total = 0; for (auto &v : st) { v = (v + 1) / 2; total += v; } }
  }
  int decode(Dec &d) {  // Decode, rc.h:403-417; -1: the cumulative frequency is not below the total (GetSym, rc.h:129-141)
    const u64 lt = d.cum(total);
    u32 x = 0, cum = 0;
    while (x < 256 && cum + st[x] <= lt) cum += st[x++];
    if (x == 256) return -1;
    d.update(st[x], cum);
    st[x] += 1; total += 1;
    while (total >= (1u << 15)) { total = 0; for (auto &v : st) { v = (v + 1) / 2; total += v; } }
    return (int)x;
  }
};
struct Worker { Model256 len[2], b0[2], b1[2], b2[2]; Enc enc; };

// ---- read ids (fqs/id.cpp) ---------------------------------------------------------------------------
// N-symbol adaptive model, all ones, adder 1, max_total 2^15 (CRangeCoderModel / CRangeCoderModelFixedSize as
// constructed in CIdCompressor::Init, id.cpp:84-105; rc.h:20-173,178-338)
struct ModelN {
  std::vector<u32> st;
  u32 total;
  explicit ModelN(u32 n = 2) : st(n, 1), total(n) {}
  void encode(Enc &e, u32 x) {
    u32 cum = 0;
    for (u32 i = 0; i < x; ++i) cum += st[i];
    e.encode(st[x], cum, total);
    st[x] += 1; total += 1;
    while (total >= (1u << 15)) { total = 0; for (auto &v : st) { v = (v + 1) / 2; total += v; } }
  }
  int decode(Dec &d) {  // Decode, rc.h:403-417; -1: the cumulative frequency is not below the total, or the stream has run out
    const u64 lt = d.cum(total);
    u32 x = 0, cum = 0;
    while (x < st.size() && cum + st[x] <= lt) cum += st[x++];
    if (x == st.size()) return -1;
    d.update(st[x], cum);
    if (d.over) return -1;
    st[x] += 1; total += 1;
    while (total >= (1u << 15)) { total = 0; for (auto &v : st) { v = (v + 1) / 2; total += v; } }
    return (int)x;
  }
};
struct CtxMap {  // exact map context -> model, created from the all-ones template on first use (id.cpp:763-811)
  u32 n;
  std::unordered_map<u64, ModelN> m;
  explicit CtxMap(u32 n_) : n(n_) {}
  ModelN &at(u64 ctx) {
    auto it = m.find(ctx);
    if (it == m.end()) it = m.emplace(ctx, ModelN(n)).first;
    return it->second;
  }
};
struct Token { u8 numeric, sep; u32 b, e; };
struct Mtf {  // classic move-to-front list of instrument names (mtf.cpp:52-116)
  std::vector<std::string> v;
  int code(const std::string &x) const {
    for (size_t i = 0; i < v.size(); ++i) if (v[i] == x) return (int)i;
    return -1;
  }
  void insert(const std::string &x) {
    int p = code(x);
    if (p < 0) { v.push_back(x); p = (int)v.size() - 1; }
    if (p > 0) { std::string s = v[p]; v.erase(v.begin() + p); v.insert(v.begin(), s); }
  }
};
struct IdWorker {
  Enc enc;
  u64 ctx_flags = 0, ctx_pe_flags = 0;
  CtxMap flags{2}, pe_flags{2}, numeric_size{256}, numeric_small{4}, literal{128}, literal_same{2}, literal_same_length{2}, plain{128};
  std::vector<Token> tok_prev, tok_cur;
  std::vector<int64_t> deltas;
  std::vector<u8> id_prev, id_cur;   // private copies: instrument mode terminates the name in place (id.cpp:427-428)
  std::vector<u8> dec_ids;           // decoder: the worker's lines of the block ...
  std::vector<u32> dec_len;          // ... and their lengths
  Mtf mtf;
  ModelN mtf_flag{11};
  std::vector<ModelN> mtf_code, mtf_byte;
  int err = 0;
  IdWorker() {
    for (int i = 0; i < 7; ++i) mtf_code.emplace_back(2u << i);
    for (int i = 0; i < 4; ++i) mtf_byte.emplace_back(256u);
  }
  void reset_read_prev() {  // CIdCompressor::ResetReadPrev, id.cpp:124-135
    id_prev.clear(); tok_prev.clear(); tok_cur.clear(); deltas.clear();
    ctx_flags = 0; ctx_pe_flags = 0;
  }
};
inline bool is_num(u8 c) { return c >= '0' && c <= '9'; }
inline bool is_lit(u8 c) { return is_num(c) || (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || c == '@'; }  // id.cpp:57-70
// tokenize, id.cpp:734-757: a token ends at every non-literal byte (kept as its separator); an all-digit token
// of 1..10 digits is numeric
void tokenize(const u8 *p, u32 size, std::vector<Token> &v) {
  u32 start = 0;
  bool numeric = true;
  v.clear();
  for (u32 i = 0; i < size; ++i) {
    if (!is_lit(p[i])) {
      if (numeric && (i - start >= 11 || i == start)) numeric = false;
      v.push_back(Token{(u8)numeric, p[i], start, i});
      numeric = true;
      start = i + 1;
    } else if (!is_num(p[i]))
      numeric = false;
  }
}
bool types_same(const std::vector<Token> &a, const std::vector<Token> &b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (a[i].numeric != b[i].numeric || a[i].sep != b[i].sep) return false;
  return true;
}
int64_t get_int(const u8 *p, u32 b, u32 e) {
  int64_t r = 0;
  for (u32 i = b; i < e; ++i) r = r * 10 + (int64_t)(p[i] - '0');
  return r;
}
u64 ilog2_(u64 x) { u64 r = 0; for (; x; ++r) x >>= 1; return r; }  // utils.h:154-162
// compress_lossless, id.cpp:257-418
void id_lossless(IdWorker &w, const u8 *p, u32 size) {
  for (u32 i = 0; i < size; ++i) if (p[i] >= 128) { w.err = 1; return; }  // 128-symbol models (id.cpp:99,104)
  w.id_cur.assign(p, p + size);
  p = w.id_cur.data();
  const u8 *q = w.id_prev.data();
  tokenize(p, size, w.tok_cur);
  const u32 n_tok = (u32)w.tok_cur.size();
  ModelN &fl = w.flags.at(w.ctx_flags);
  if (types_same(w.tok_cur, w.tok_prev)) {
    fl.encode(w.enc, 1);
    w.ctx_flags = ((w.ctx_flags << 1) + 1) & 0xff;
    for (u32 i = 0; i < n_tok; ++i) {
      const Token &c = w.tok_cur[i], &pv = w.tok_prev[i];
      if (!c.numeric) {
        const u32 len = c.e - c.b;
        const bool same_length = len == pv.e - pv.b;
        const bool same = same_length && std::equal(p + c.b, p + c.e, q + pv.b);
        ModelN &ms = w.literal_same.at(i);
        if (same) { ms.encode(w.enc, 1); continue; }
        ms.encode(w.enc, 0);
        ModelN &ml = w.literal_same_length.at(i);
        if (same_length) {
          ml.encode(w.enc, 1);
          for (u32 j = 0; j < len; ++j) {
            ModelN &m = w.literal.at(w.ctx_flags + (1ull << 32) + j);
            m.encode(w.enc, p[c.b + j] == q[pv.b + j] ? 0u : (u32)p[c.b + j]);
          }
        } else {
          ml.encode(w.enc, 0);
          for (u32 j = 0; j < len; ++j) w.literal.at(w.ctx_flags + j).encode(w.enc, p[c.b + j]);
          w.literal.at(w.ctx_flags + len).encode(w.enc, 0);
        }
      } else {
        int64_t delta = get_int(p, c.b, c.e) - get_int(q, pv.b, pv.e);
        const int64_t d0 = w.deltas[i];
        u64 ctx = (u64)i << 40;
        ctx += ilog2_((u64)(d0 < 0 ? -d0 : d0)) << 31;
        ctx += (u64)(d0 < 0) << 30;
        ModelN &msz = w.numeric_size.at(ctx);
        ModelN &msm = w.numeric_small.at(ctx);
        w.deltas[i] = delta;
        if (delta >= -1 && delta <= 1) { msm.encode(w.enc, (u32)(delta + 1)); continue; }
        msm.encode(w.enc, 3);
        int n_bytes = 0;
        if (delta >= -123 && delta <= 123) msz.encode(w.enc, (u32)(delta + 123) & 0xff);
        else if (delta > 0 && delta < 0x10000ll) { msz.encode(w.enc, 247); n_bytes = 2; ctx += 0x10; }
        else if (delta > 0 && delta < 0x1000000ll) { msz.encode(w.enc, 248); n_bytes = 3; ctx += 0x20; }
        else if (delta > 0 && delta < 0x100000000ll) { msz.encode(w.enc, 249); n_bytes = 4; ctx += 0x30; }
        else if (delta > 0) { msz.encode(w.enc, 250); n_bytes = 8; ctx += 0x40; }
        else if (delta > -0x10000ll) { msz.encode(w.enc, 251); delta = -delta; n_bytes = 2; ctx += 0x50; }
        else if (delta > -0x1000000ll) { msz.encode(w.enc, 252); delta = -delta; n_bytes = 3; ctx += 0x60; }
        else if (delta > -0x100000000ll) { msz.encode(w.enc, 253); delta = -delta; n_bytes = 4; ctx += 0x70; }
        else { msz.encode(w.enc, 254); delta = -delta; n_bytes = 8; ctx += 0x80; }
        for (int j = 0; j < n_bytes; ++j) w.numeric_size.at(ctx + j).encode(w.enc, (u32)(((u64)delta >> (8 * j)) & 0xff));
      }
    }
  } else {
    fl.encode(w.enc, 0);
    w.ctx_flags = (w.ctx_flags << 1) & 0xff;
    for (u32 i = 0; i < size; ++i) w.plain.at(i).encode(w.enc, p[i]);
    w.deltas.assign(n_tok, 0);
  }
  w.tok_prev.swap(w.tok_cur);
  w.id_prev.swap(w.id_cur);
}
// compress_instrument, id.cpp:421-495: only the instrument name (up to the first '.', ' ' or ':') is kept
void id_instrument(IdWorker &w, const u8 *p, u32 size) {
  u32 n = 0;
  while (n < size && p[n] != '.' && p[n] != ' ' && p[n] != ':') ++n;
  if (n == size) { w.err = 2; return; }  // the reference would write its terminator over the first base here
  std::string name((const char *)p, n);
  name = std::string(name.c_str());      // std::string(char*) stops at an embedded NUL (id.cpp:428)
  int code = w.mtf.code(name);
  if (code < 0) {
    w.mtf_flag.encode(w.enc, 0);
    std::vector<u8> tmp(p, p + n);
    tmp.push_back(0);
    id_lossless(w, tmp.data(), n + 1);
  } else if (code < 2)
    w.mtf_flag.encode(w.enc, (u32)code + 1);
  else if (code < 256) {
    int k = 0;
    while ((4 << k) <= code) ++k;          // code in [2<<k, 4<<k)
    w.mtf_flag.encode(w.enc, 3 + k);
    w.mtf_code[k].encode(w.enc, (u32)code - (2u << k));
  } else {
    w.mtf_flag.encode(w.enc, 10);
    for (int i = 0; i < 4; ++i) { w.mtf_byte[i].encode(w.enc, (u32)code & 0xff); code >>= 8; }
  }
  w.mtf.insert(name);
}
bool typical_pe_ids(const u8 *a, u32 na, const u8 *b, u32 nb) {  // id.cpp:241-254
  if (na != nb || na < 3) return false;
  if (!std::equal(a, a + na - 2, b)) return false;
  return a[na - 2] == '1' && b[nb - 2] == '2';
}

// ---- the decoder (id.cpp:182-228, 495-731).  No limits on a line beyond the format's; a malformed stream ends in w.err.
const size_t ID_LINE_LIMIT = 1u << 24;   // (a line the reference's block buffer could not hold either)
// store_int, id.h:117-149: one digit below 10 (also for negative values, whose "digit" is '0' + val % 10), none from 10^15
void store_int(std::vector<u8> &p, int64_t val) {
  int n_dig = 0;
  if (val < 1000000000000000ll) {
    n_dig = 1;
    for (int64_t t = 10; n_dig < 15 && val >= t; t *= 10) ++n_dig;
  }
  const size_t begin = p.size();
  p.resize(begin + n_dig);
  for (int i = n_dig - 1; i >= 0; --i) { p[begin + i] = (u8)('0' + (int)(val % 10)); val /= 10; }
}
// decompress_lossless, id.cpp:495-666: the line is left in w.id_prev
void id_dec_lossless(IdWorker &w, Dec &d) {
  std::vector<u8> &p = w.id_cur;
  p.clear();
  auto sym = [&](ModelN &m) -> u32 { const int x = m.decode(d); if (x < 0) { w.err = 7; return 0; } return (u32)x; };
  if (sym(w.flags.at(w.ctx_flags)) == 1 && !w.err) {   // tokens of the same type
    w.ctx_flags = ((w.ctx_flags << 1) + 1) & 0xff;
    const u32 n_tok = (u32)w.tok_prev.size();
    if (w.deltas.size() < n_tok) w.deltas.resize(n_tok, 0);
    const u8 *q = w.id_prev.data();
    for (u32 i = 0; i < n_tok && !w.err; ++i) {
      const Token &pv = w.tok_prev[i];
      if (!pv.numeric) {
        if (sym(w.literal_same.at(i)) == 1) p.insert(p.end(), q + pv.b, q + pv.e);
        else if (w.err) break;
        else if (sym(w.literal_same_length.at(i)) == 1) {
          for (u32 j = 0; j < pv.e - pv.b && !w.err; ++j) {
            // !!! Fix mixing literal contexts (id.cpp:525)
            const u32 c = sym(w.literal.at(w.ctx_flags + (1ull << 32) + j));
            p.push_back(c == 0 ? q[pv.b + j] : (u8)c);
          }
        } else {
          for (u32 j = 0; !w.err; ++j) {
            const u32 c = sym(w.literal.at(w.ctx_flags + j));
            if (!c) break;
            p.push_back((u8)c);
            if (p.size() > ID_LINE_LIMIT) w.err = 5;
          }
        }
      } else {
        const int64_t v_prev = get_int(q, pv.b, pv.e), d0 = w.deltas[i];
        u64 ctx = (u64)i << 40;
        ctx += ilog2_(d0 < 0 ? 0ull - (u64)d0 : (u64)d0) << 31;
        ctx += (u64)(d0 < 0) << 30;
        ModelN &msz = w.numeric_size.at(ctx);
        ModelN &msm = w.numeric_small.at(ctx);
        int64_t delta;
        u32 c = sym(msm);
        if (w.err) break;
        if (c < 3) delta = (int64_t)c - 1;
        else {
          int n_bytes = 0;
          u64 ud = 0;
          c = sym(msz);
          if (w.err) break;
          if (c <= 246) ud = (u64)((int64_t)c - 123);
          else if (c == 247) { n_bytes = 2; ctx += 0x10; }
          else if (c == 248) { n_bytes = 3; ctx += 0x20; }
          else if (c == 249) { n_bytes = 4; ctx += 0x30; }
          else if (c == 250) { n_bytes = 8; ctx += 0x40; }
          else if (c == 251) { n_bytes = 2; ctx += 0x50; }
          else if (c == 252) { n_bytes = 3; ctx += 0x60; }
          else if (c == 253) { n_bytes = 4; ctx += 0x70; }
          else if (c == 254) { n_bytes = 8; ctx += 0x80; }
          for (int j = 0; j < n_bytes && !w.err; ++j) ud += (u64)sym(w.numeric_size.at(ctx + j)) << (8 * j);
          if (c >= 251) ud = 0ull - ud;
          delta = (int64_t)ud;
        }
        w.deltas[i] = delta;
        store_int(p, (int64_t)((u64)delta + (u64)v_prev));
      }
      p.push_back(pv.sep);
    }
    if (w.err) return;
    tokenize(p.data(), (u32)p.size(), w.tok_cur);
  } else {
    if (w.err) return;
    w.ctx_flags = (w.ctx_flags << 1) & 0xff;
    for (u32 i = 0;; ++i) {   // decode id plain
      const u32 c = sym(w.plain.at(i));
      if (w.err) return;
      p.push_back((u8)c);
      if (c == 0 || c == 0x0A) break;
      if (p.size() > ID_LINE_LIMIT) { w.err = 5; return; }
    }
    tokenize(p.data(), (u32)p.size(), w.tok_cur);
    w.deltas.assign(w.tok_cur.size(), 0);
  }
  w.tok_prev.swap(w.tok_cur);
  w.id_prev.swap(w.id_cur);
}
// decompress_instrument, id.cpp:669-731: the instrument name and a line feed are appended to `out`
void id_dec_instrument(IdWorker &w, Dec &d, std::vector<u8> &out) {
  auto sym = [&](ModelN &m) -> u32 { const int x = m.decode(d); if (x < 0) { w.err = 7; return 0; } return (u32)x; };
  const u32 flag = sym(w.mtf_flag);
  if (w.err) return;
  if (flag == 0) {   // new instrument name
    id_dec_lossless(w, d);
    if (w.err) return;
    const std::vector<u8> &p = w.id_prev;
    if (p.empty()) { w.err = 7; return; }
    const std::string name(p.begin(), std::find(p.begin(), p.end(), (u8)0));
    out.insert(out.end(), p.begin(), p.end());
    out.back() = '\n';
    w.mtf.insert(name);
    return;
  }
  u32 code = 0;
  if (flag < 3) code = flag - 1;
  else if (flag < 10) code = sym(w.mtf_code[flag - 3]) + (2u << (flag - 3));
  else
    for (int i = 0; i < 4 && !w.err; ++i) code += sym(w.mtf_byte[i]) << (8 * i);
  if (w.err) return;
  if (code >= w.mtf.v.size()) { w.err = 7; return; }
  if (code > 0) { std::string s = w.mtf.v[code]; w.mtf.v.erase(w.mtf.v.begin() + code); w.mtf.v.insert(w.mtf.v.begin(), s); }   // mtf.Insert(code)
  const std::string &s = w.mtf.v[0];
  out.insert(out.end(), s.begin(), s.end());
  out.push_back('\n');
}
}  // namespace

struct fqsx_meta { u32 T; std::vector<Worker> w; };
struct fqsx_id { u32 T, mode; std::vector<IdWorker> w; std::vector<u8> ids; std::vector<u64> off; };

extern "C" {
// Per-bin read order of `fqs e -om s`: std::sort with the comparator of CSortedFASTQFile::sort_reads
// (fqs/io.h:499-528) on the reads in their input order.  The sort is unstable; using the same libstdc++
// algorithm on the same initial sequence reproduces the reference's order of reads that compare equal
// (identical DNA), which matters for paired-end data (the mates follow this order, io.h:541-550).
int fqsx_sort_bin(const uint8_t *bases, const uint64_t *off, const uint32_t *idx_in, uint32_t n, uint32_t *idx_out) {
  if (!bases || !off || !idx_in || !idx_out) return FQSX_E_ARG;
  struct R { const u8 *p; u32 len; u32 id; };
  std::vector<R> v(n);
  for (u32 i = 0; i < n; ++i) v[i] = R{bases + off[idx_in[i]], (u32)(off[idx_in[i] + 1] - off[idx_in[i]]), idx_in[i]};
  auto nt = [](u8 c) -> int { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3; };
  std::sort(v.begin(), v.end(), [&](const R &x, const R &y) {
    u32 m = x.len < y.len ? x.len : y.len;
    for (u32 i = 0; i < m; ++i) {
      int a = nt(x.p[i]), b = nt(y.p[i]);
      if (a != b) return a < b;
    }
    if (x.len != y.len) return x.len < y.len;
    for (u32 i = 0; i < m; ++i)
      if (x.p[i] != y.p[i]) return x.p[i] < y.p[i];
    return false;
  });
  for (u32 i = 0; i < n; ++i) idx_out[i] = v[i].id;
  return FQSX_OK;
}
int fqsx_meta_create(uint32_t T, fqsx_meta **out) {
  if (!out || T == 0 || T > 255) return FQSX_E_ARG;
  fqsx_meta *m = new fqsx_meta;
  m->T = T;
  m->w.resize(T);
  *out = m;
  return FQSX_OK;
}
void fqsx_meta_destroy(fqsx_meta *m) { delete m; }
static int encode_len(Worker &w, u32 mdl, u32 L) {  // encode_len(model, len), meta.cpp:48-73
  if (L < 254) w.len[mdl].encode(w.enc, L);
  else if (L < 65536) { w.len[mdl].encode(w.enc, 254); w.b1[mdl].encode(w.enc, L >> 8); w.b2[mdl].encode(w.enc, L & 0xff); }
  else if (L < (1u << 24)) { w.len[mdl].encode(w.enc, 255); w.b0[mdl].encode(w.enc, L >> 16); w.b1[mdl].encode(w.enc, (L >> 8) & 0xff); w.b2[mdl].encode(w.enc, L & 0xff); }
  else return FQSX_E_ARG;
  return FQSX_OK;
}
int fqsx_meta_encode_block_pe(fqsx_meta *m, const uint32_t *read_len, uint32_t n_reads, int paired, const uint8_t **streams, uint64_t *lens);
int fqsx_meta_encode_block(fqsx_meta *m, const uint32_t *read_len, uint32_t n_reads, const uint8_t **streams, uint64_t *lens) {
  return fqsx_meta_encode_block_pe(m, read_len, n_reads, 0, streams, lens);
}
// paired: reads alternate mate 1 / mate 2 and use models 0 / 1 (CompressReadLenPE, meta.cpp:100-107)
int fqsx_meta_encode_block_pe(fqsx_meta *m, const uint32_t *read_len, uint32_t n_reads, int paired, const uint8_t **streams, uint64_t *lens) {
  if (!m || !read_len || !streams || !lens) return FQSX_E_ARG;
  const u64 T = m->T;
  for (u64 t = 0; t < T; ++t) {
    u64 first, last;
    worker_reads(t, T, n_reads, first, last);
    Worker &w = m->w[t];
    w.enc.start();
    for (u64 i = first; i < last; ++i)
      if (encode_len(w, paired ? (u32)((i - first) & 1) : 0u, read_len[i])) return FQSX_E_ARG;
    w.enc.end();
    streams[t] = w.enc.out.data();
    lens[t] = w.enc.out.size();
  }
  return FQSX_OK;
}
// decode_len(model), meta.cpp:76-97; false: malformed stream
static bool decode_len(Worker &w, Dec &d, u32 mdl, u32 &L) {
  const int flag = w.len[mdl].decode(d);
  if (flag < 0) return false;
  if (flag < 254) { L = (u32)flag; return true; }
  int b0 = 0, b1, b2;
  if (flag == 255 && (b0 = w.b0[mdl].decode(d)) < 0) return false;
  if ((b1 = w.b1[mdl].decode(d)) < 0 || (b2 = w.b2[mdl].decode(d)) < 0) return false;
  L = ((u32)b0 << 16) + ((u32)b1 << 8) + (u32)b2;
  return true;
}
// inverse of fqsx_meta_encode_block_pe (DecompressReadLen / DecompressReadLenPE, meta.cpp:108-131)
int fqsx_meta_decode_block(fqsx_meta *m, const uint8_t *const *streams, const uint64_t *lens, uint32_t n_reads, int paired,
                           uint32_t *read_len_out) {
  if (!m || !streams || !lens || !read_len_out) return FQSX_E_ARG;
  const u64 T = m->T;
  for (u64 t = 0; t < T; ++t) {
    u64 first, last;
    worker_reads(t, T, n_reads, first, last);
    if (first == last) continue;
    if (!streams[t] || lens[t] < 8) return FQSX_E_ARG;   // sub_rc.h:114
    Worker &w = m->w[t];
    Dec d;
    d.start(streams[t], lens[t]);
    for (u64 i = first; i < last; ++i)
      if (!decode_len(w, d, paired ? (u32)((i - first) & 1) : 0u, read_len_out[i]) || d.over) return FQSX_E_ARG;   // ran out of bytes
  }
  return FQSX_OK;
}

// ---- read ids: CIdCompressor::Compress / CompressPE for all T workers of one block ----------------------
int fqsx_id_create(const uint8_t *header17, fqsx_id **out) {
  if (!header17 || !out || memcmp(header17, "KCSD", 4) || header17[4] == 0 || header17[7] > 2) return FQSX_E_ARG;
  fqsx_id *h = new fqsx_id;
  h->T = header17[4];
  h->mode = header17[7];   // 0 lossless, 1 instrument, 2 none (params.h:18,92)
  h->w.resize(h->T);
  *out = h;
  return FQSX_OK;
}
void fqsx_id_destroy(fqsx_id *h) { delete h; }
// ids: concatenated id lines, each INCLUDING its '\n' (read_desc_t::id_len, defs.h:70-72); id_off: n_reads+1
// offsets; paired != 0: reads alternate mate 1 / mate 2.  Workers are independent (no shared state), so they
// run on host threads.
int fqsx_id_encode_block(fqsx_id *h, const uint8_t *ids, const uint64_t *id_off, uint32_t n_reads, int paired,
                         const uint8_t **streams, uint64_t *lens) {
  if (!h || !ids || !id_off || !streams || !lens || (paired && (n_reads & 1))) return FQSX_E_ARG;
  const u64 T = h->T;
  auto run = [&](u64 t) {
    u64 first, last;
    worker_reads(t, T, n_reads, first, last);
    IdWorker &w = h->w[t];
    w.reset_read_prev();
    w.enc.start();
    if (h->mode != 2)
      for (u64 i = first; i < last && !w.err; i += paired ? 2 : 1) {
        const u8 *p1 = ids + id_off[i];
        const u32 n1 = (u32)(id_off[i + 1] - id_off[i]);
        if (!paired) {
          if (h->mode == 0) id_lossless(w, p1, n1); else id_instrument(w, p1, n1);
          continue;
        }
        const u8 *p2 = ids + id_off[i + 1];
        const u32 n2 = (u32)(id_off[i + 2] - id_off[i + 1]);
        if (h->mode == 0) {   // CompressPE, id.cpp:152-184
          ModelN &m = w.pe_flags.at(w.ctx_pe_flags);
          const bool typical = typical_pe_ids(p1, n1, p2, n2);
          w.ctx_pe_flags = ((w.ctx_pe_flags << 1) + (typical ? 1 : 0)) & 0xff;
          m.encode(w.enc, typical ? 1 : 0);
          id_lossless(w, p1, n1);
          if (!typical) id_lossless(w, p2, n2);
        } else {
          id_instrument(w, p1, n1);
          id_instrument(w, p2, n2);
        }
      }
    w.enc.end();
  };
  const u32 nthr = (u32)std::max<u64>(1, std::min<u64>(T, std::thread::hardware_concurrency()));
  if (nthr <= 1 || n_reads < 4096) for (u64 t = 0; t < T; ++t) run(t);
  else {
    std::vector<std::thread> th;
    for (u32 k = 0; k < nthr; ++k) th.emplace_back([&, k] { for (u64 t = k; t < T; t += nthr) run(t); });
    for (auto &x : th) x.join();
  }
  for (u64 t = 0; t < T; ++t) {
    if (h->w[t].err) return FQSX_E_ARG;
    streams[t] = h->w[t].enc.out.data();
    lens[t] = h->w[t].enc.out.size();
  }
  return FQSX_OK;
}

// Inverse of fqsx_id_encode_block: CIdCompressor::Decompress / DecompressPE (id.cpp:182-228) for all T workers of one block.
// The lines are what the reference's `fqs d` writes (numeric fields rebuilt by store_int, instrument mode: name + line feed).
int fqsx_id_decode_block(fqsx_id *h, const uint8_t *const *streams, const uint64_t *lens, uint32_t n_reads, int paired,
                         const uint8_t **ids_out, const uint64_t **id_off_out) {
  if (!h || !streams || !lens || !ids_out || !id_off_out || (paired && (n_reads & 1))) return FQSX_E_ARG;
  const u64 T = h->T;
  for (u64 t = 0; t < T; ++t) {
    u64 first, last;
    worker_reads(t, T, n_reads, first, last);
    if (h->mode != 2 && first < last && (!streams[t] || lens[t] < 8)) return FQSX_E_ARG;   // sub_rc.h:114
  }
  auto run = [&](u64 t) {
    u64 first, last;
    worker_reads(t, T, n_reads, first, last);
    IdWorker &w = h->w[t];
    w.reset_read_prev();
    std::vector<u8> &out = w.dec_ids;
    out.clear(); w.dec_len.clear();
    if (first == last) return;
    if (h->mode == 2) {   // decompress_none, id.cpp:486-492
      for (u64 i = first; i < last; ++i) { out.push_back('@'); out.push_back('\n'); w.dec_len.push_back(2); }
      return;
    }
    Dec d;
    d.start(streams[t], lens[t]);
    auto line = [&] {   // one id through the mode's decoder, appended to `out`
      const size_t at = out.size();
      if (h->mode == 0) { id_dec_lossless(w, d); if (!w.err) out.insert(out.end(), w.id_prev.begin(), w.id_prev.end()); }
      else id_dec_instrument(w, d, out);
      w.dec_len.push_back((u32)(out.size() - at));
    };
    for (u64 i = first; i < last && !w.err; i += paired ? 2 : 1) {
      if (!paired || h->mode != 0) { line(); if (paired && !w.err) line(); continue; }
      const int typical = w.pe_flags.at(w.ctx_pe_flags).decode(d);   // DecompressPE, id.cpp:195-228
      if (typical < 0) { w.err = 7; break; }
      w.ctx_pe_flags = ((w.ctx_pe_flags << 1) + (u64)typical) & 0xff;
      line();
      if (w.err) break;
      if (typical) {   // typical PE ids: mate 2 is mate 1 with the byte before the line feed set to '2'
        const size_t n = w.dec_len.back(), at = out.size();
        const std::vector<u8> mate1(out.end() - n, out.end());
        out.insert(out.end(), mate1.begin(), mate1.end());
        if (n >= 2) out[at + n - 2] = '2';
        w.dec_len.push_back((u32)n);
      } else
        line();
    }
  };
  const u32 nthr = (u32)std::max<u64>(1, std::min<u64>(T, std::thread::hardware_concurrency()));
  if (nthr <= 1 || n_reads < 4096) for (u64 t = 0; t < T; ++t) run(t);
  else {
    std::vector<std::thread> th;
    for (u32 k = 0; k < nthr; ++k) th.emplace_back([&, k] { for (u64 t = k; t < T; t += nthr) run(t); });
    for (auto &x : th) x.join();
  }
  h->ids.clear();
  h->off.assign(1, 0);
  for (u64 t = 0; t < T; ++t) {
    if (h->w[t].err) return FQSX_E_DEVICE;   // malformed or truncated stream (the code the GPU decoder gives it)
    h->ids.insert(h->ids.end(), h->w[t].dec_ids.begin(), h->w[t].dec_ids.end());
    for (u32 n : h->w[t].dec_len) h->off.push_back(h->off.back() + n);
  }
  if (h->off.size() != (size_t)n_reads + 1) return FQSX_E_DEVICE;
  h->ids.resize(h->ids.size() + 8);   // (never a null pointer for an empty block)
  *ids_out = h->ids.data();
  *id_off_out = h->off.data();
  return FQSX_OK;
}

// The gzip member headers of buf[0 .. n_bytes) as bgzip writes them (RFC 1952; SAM specification, section 4.1): magic 1f 8b,
// CM 8, FLG = FEXTRA, XLEN at byte 10, among the extra subfields `BC` with a 2-byte BSIZE = member size - 1; the deflate data
// lies between the 12 + XLEN header bytes and the 8 trailer bytes (CRC-32, ISIZE).  The walk ends at the first member that is
// not whole in the buffer, at max_members, or at bytes that are no such header.
int fqsx_bgzf_scan(const uint8_t *buf, uint64_t n_bytes, uint32_t max_members, uint64_t *member_off, uint32_t *isize, uint64_t out[4]) {
  if (!out || (n_bytes && !buf) || (max_members && (!member_off || !isize))) return FQSX_E_ARG;
  u64 pos = 0, n = 0, not_bgzf = 0;
  while (n < max_members && pos < n_bytes) {
    const u8 *h = buf + pos;
    const u64 left = n_bytes - pos;
    // (what is there of the fixed part decides as early as it can: a file that is no BGZF is told from its first bytes)
    static const u8 want[4] = {0x1f, 0x8b, 8, 4};
    bool bad = false;
    for (u32 k = 0; k < 4 && k < left; ++k) bad |= k < 3 ? h[k] != want[k] : (h[k] & 0x1eu) != want[k];
    if (bad) { not_bgzf = 1; break; }
    if (left < 12) break;
    const u64 xlen = (u64)h[10] | ((u64)h[11] << 8);
    if (left < 12 + xlen) break;
    u64 bsize = 0, q = 12;
    bool found = false;
    while (q + 4 <= 12 + xlen) {
      const u64 slen = (u64)h[q + 2] | ((u64)h[q + 3] << 8);
      if (h[q] == 'B' && h[q + 1] == 'C' && slen == 2 && q + 6 <= 12 + xlen) {
        bsize = ((u64)h[q + 4] | ((u64)h[q + 5] << 8)) + 1;
        found = true;
        break;
      }
      q += 4 + slen;
    }
    if (!found || bsize < 12 + xlen + 8) { not_bgzf = 1; break; }
    if (left < bsize) break;
    member_off[n] = pos;
    isize[n] = (u32)h[bsize - 4] | ((u32)h[bsize - 3] << 8) | ((u32)h[bsize - 2] << 16) | ((u32)h[bsize - 1] << 24);
    n += 1;
    pos += bsize;
  }
  out[0] = n;
  out[1] = pos;
  out[2] = n_bytes - pos;
  out[3] = not_bgzf;
  return FQSX_OK;
}
}
