// fqsx_inflate.h -- BGZF members to text on the GPU: the inflate stage in front of the FASTQ parser.
//
// A BGZF file is gzip cut into members that do not depend on one another: each holds at most 64 KiB of text as one raw
// DEFLATE stream (RFC 1951) between a gzip header with a `BC` extra subfield and the CRC-32 / ISIZE trailer (RFC 1952).
// k_bgzf_inflate gives every member one wavefront (= one workgroup) and writes its text at the member's offset of the
// chunk the parser reads:
//   - the symbols are decoded with wave-uniform control flow (bit buffer, positions and the block state are the same in
//     all lanes); the lanes do the wide work: the compressed bytes come into LDS 1 KiB at a time, the code-length counts
//     are cleared and the lookup tables filled across the lanes, a match is copied as out[p + k] = out[p - d + (k mod d)]
//     over k, and the copy-out and the CRC run over all lanes;
//   - the member's output window lies in LDS beside the tables (74 KiB in all: two members per compute unit), shifted so
//     that a 16-byte step of the window is a 16-byte step of the text; the LDS operations of one wave stay in order, so
//     a match that reads what other lanes have just written needs no more than FQ_SYNC; the window leaves for global
//     memory once, in 16-byte stores, after its CRC-32 (64 slices, one per lane, joined by the shifts x^(8 len) mod P)
//     and its size have been checked;
//   - every loop is bounded by the member's input bits and by its ISIZE: nothing outside the member's compressed bytes
//     is read, nothing outside its ISIZE bytes of the text is written, whatever the bytes say.  A damaged member ends
//     with a kind (INF_E_*) in its status word and leaves its text unwritten.
// What is accepted is what zlib's inflate accepts (inftrees.c: an over-subscribed code is refused; an incomplete one too
// unless it is a literal/length or distance code of a single 1-bit code; a block needs its end-of-block code).
#pragma once
#include "fqsx_plat.h"

#define INF_WINDOW 65536u        // most text a member holds
#define INF_CHUNK 1024u          // compressed bytes staged in LDS at a time
#define INF_FAST 10u             // bits the lookup tables resolve; longer codes walk the canonical counts
#define INF_SLICES 64u           // CRC slices of a member (one per lane on the GPU)
enum {
  INF_OK = 0,
  INF_E_BTYPE = 1,       // reserved block type
  INF_E_STORED = 2,      // stored LEN / NLEN mismatch
  INF_E_CODE = 3,        // over-subscribed or incomplete code, too many codes, no end-of-block code
  INF_E_SYMBOL = 4,      // invalid symbol (unused code, literal/length 286-287, distance 30-31, a repeat without a length before it or beyond the lengths)
  INF_E_DISTANCE = 5,    // distance before the member's start
  INF_E_OUTPUT = 6,      // output beyond ISIZE
  INF_E_INPUT = 7,       // input exhausted
  INF_E_ISIZE = 8,       // ISIZE mismatch
  INF_E_CRC = 9,         // CRC mismatch
  INF_E_HEADER = 10,     // no gzip member header with room for a trailer
  INF_N_KINDS
};

struct InfCfg {
  const u8 *in;         // the members back to back
  const u64 *in_off;    // [n + 1]
  u8 *out;              // the chunk's text; 16-byte aligned
  const u64 *out_off;   // [n + 1]: where each member's text goes (differences: the ISIZE the host read, at most INF_WINDOW)
  u64 out_cap;          // bytes of out
  u32 *status;          // [n]
  u32 n;
};

struct alignas(16) Inf16 { u64 lo, hi; };

struct InfLds {
  Inf16 win[(INF_WINDOW + 16) / 16];
  u32 inw[INF_CHUNK / 4];
  u32 crc_tab[256];
  u16 lfast[1u << INF_FAST], dfast[1u << INF_FAST];   // (symbol << 4) | length, 0: not resolved here
  u16 lsym[288], dsym[32];                            // symbols in canonical order
  u32 lcount[16], dcount[16];                        // codes of every length
  u16 next[16], offs[16];                             // per length, while a table is built: the next code, the next place in the order
  u16 code[320];                                      // canonical code of every symbol while a table is built
  u8 lens[320];
};

struct InfState {   // wave-uniform
  const u8 *in;
  u64 ip, iend, cb;   // next byte to take, end of the deflate data, first byte of the staged chunk
  u64 bits;
  u32 nbits;
  u32 op, out_len;
};

FQ_DEV u32 inf_min32(u32 a, u32 b) { return a < b ? a : b; }

// the chunk that starts at s.ip into LDS (zeros behind the data's end)
FQ_DEV void inf_stage(InfLds &L, InfState &s) {
  s.cb = s.ip;
  u8 *b = (u8 *)L.inw;
  for (u32 k = FQ_LANE; k < INF_CHUNK; k += FQ_WAVE) b[k] = s.cb + k < s.iend ? s.in[s.cb + k] : (u8)0;
  FQ_SYNC();
}
// at least 33 bits in the buffer unless the data ends before
FQ_DEV void inf_refill(InfLds &L, InfState &s) {
  if (s.nbits > 32 || s.ip >= s.iend) return;
  if (s.ip - s.cb >= INF_CHUNK) inf_stage(L, s);
  const u32 k = (u32)(s.iend - s.ip < 4 ? s.iend - s.ip : 4);
  s.bits |= (u64)uniform32(L.inw[(s.ip - s.cb) >> 2]) << s.nbits;
  s.nbits += 8 * k;
  s.ip += k;
}
// n <= 16 bits; false: the data has ended
FQ_DEV bool inf_take(InfLds &L, InfState &s, u32 n, u32 &v) {
  inf_refill(L, s);
  if (s.nbits < n) return false;
  v = (u32)(s.bits & ((1ull << n) - 1ull));
  s.bits >>= n;
  s.nbits -= n;
  return true;
}

// Counts, canonical order and lookup table of the code with lengths lens[0 .. n).  kind: the code-length code, a
// literal/length code or a distance code (which alone may be empty).
enum { INF_CODES = 0, INF_LENS = 1, INF_DISTS = 2 };
FQ_DEV u32 inf_build(InfLds &L, const u8 *lens, u32 n, u32 kind, u32 *count, u16 *sym, u16 *fast) {
  for (u32 k = FQ_LANE; k < (1u << INF_FAST); k += FQ_WAVE) fast[k] = 0;
  for (u32 k = FQ_LANE; k < 16; k += FQ_WAVE) count[k] = 0;
  FQ_SYNC();
  for (u32 i = FQ_LANE; i < n; i += FQ_WAVE)
    if (lens[i] & 15u) lds_inc32(&count[lens[i] & 15u]);
  FQ_SYNC();
  u32 err = INF_OK;
  if (FQ_LANE == 0) {
    u32 max = 15;
    while (max && !count[max]) --max;
    i32 left = 1;
    u32 c = 0, o = 0, before = 0;
    for (u32 l = 1; l < 16; ++l) {
      const u32 cl = count[l];
      if (left >= 0) left = left * 2 - (i32)cl;
      c = (c + before) << 1;
      L.next[l] = (u16)c;
      L.offs[l] = (u16)o;
      o += cl;
      before = cl;
    }
    if (left < 0) err = INF_E_CODE;
    else if (max == 0) err = kind == INF_DISTS ? INF_OK : INF_E_CODE;
    else if (left > 0 && (kind == INF_CODES || max != 1)) err = INF_E_CODE;
    if (!err)
      for (u32 i = 0; i < n; ++i) {
        const u32 l = lens[i] & 15u;
        if (!l) continue;
        L.code[i] = L.next[l]++;
        sym[L.offs[l]++] = (u16)i;
      }
  }
  FQ_SYNC();
  err = uniform32(err);
  if (err) return err;
  for (u32 i = FQ_LANE; i < n; i += FQ_WAVE) {
    const u32 l = lens[i] & 15u;
    if (!l || l > INF_FAST) continue;
    u32 r = 0;
    for (u32 b = 0, c = L.code[i]; b < l; ++b, c >>= 1) r = (r << 1) | (c & 1u);
    for (u32 k = r; k < (1u << INF_FAST); k += 1u << l) fast[k] = (u16)((i << 4) | l);
  }
  FQ_SYNC();
  return INF_OK;
}

// the next symbol of a code; INF_E_INPUT / INF_E_SYMBOL
FQ_DEV u32 inf_symbol(InfLds &L, InfState &s, const u32 *count, const u16 *sym, const u16 *fast, u32 &out) {
  inf_refill(L, s);
  const u32 e = uniform32(fast[s.bits & ((1u << INF_FAST) - 1u)]);
  if (e) {
    const u32 l = e & 15u;
    if (l > s.nbits) return INF_E_INPUT;
    s.bits >>= l;
    s.nbits -= l;
    out = e >> 4;
    return INF_OK;
  }
  u32 code = 0, first = 0, index = 0;
  for (u32 l = 1; l < 16; ++l) {
    if (l > s.nbits) return INF_E_INPUT;
    code |= (u32)(s.bits >> (l - 1)) & 1u;
    const u32 c = uniform32(count[l]);
    if (code < first + c) {
      s.bits >>= l;
      s.nbits -= l;
      out = uniform32(sym[index + (code - first)]);
      return INF_OK;
    }
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  return INF_E_SYMBOL;
}

FQ_DEV u32 inf_len_base(u32 k) {   // length symbol 257 + k: base | extra bits << 16
  return k < 8 ? 3 + k : k == 28 ? 258 : ((((k - 4) & 3u) + 4) << ((k - 4) >> 2)) + 3 + (((k - 4) >> 2) << 16);
}
FQ_DEV u32 inf_dist_base(u32 k) {
  return k < 4 ? 1 + k : (((k & 1u) + 2) << ((k >> 1) - 1)) + 1 + (((k >> 1) - 1) << 16);
}

// the code lengths of a dynamic block into L.lens, the two tables built
FQ_DEV u32 inf_dynamic(InfLds &L, InfState &s) {
  u32 hlit, hdist, hclen, v;
  if (!inf_take(L, s, 5, hlit) || !inf_take(L, s, 5, hdist) || !inf_take(L, s, 4, hclen)) return INF_E_INPUT;
  hlit += 257; hdist += 1; hclen += 4;
  if (hlit > 286 || hdist > 30) return INF_E_CODE;
  for (u32 k = FQ_LANE; k < 320; k += FQ_WAVE) L.lens[k] = 0;
  FQ_SYNC();
  for (u32 k = 0; k < hclen; ++k) {
    if (!inf_take(L, s, 3, v)) return INF_E_INPUT;
    const u32 order = k < 3 ? 16 + k : k == 3 ? 0 : (k & 1u) ? 7 - ((k - 5) >> 1) : 8 + ((k - 4) >> 1);   // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
    if (FQ_LANE == 0) L.lens[order] = (u8)v;
  }
  FQ_SYNC();
  // (the code-length code: built in the distance table's place, which is filled afterwards)
  u32 err = inf_build(L, L.lens, 19, INF_CODES, L.dcount, L.dsym, L.dfast);
  if (err) return err;
  u8 *ll = L.lens;   // (the code-length code's own lengths are in its table now)
  u32 have = 0, prev = 0;
  while (have < hlit + hdist) {
    u32 sy;
    if ((err = inf_symbol(L, s, L.dcount, L.dsym, L.dfast, sy))) return err;
    if (sy < 16) {
      if (FQ_LANE == 0) ll[have] = (u8)sy;
      prev = sy;
      have += 1;
      continue;
    }
    u32 rep, len = 0;
    if (sy == 16) {
      if (!have) return INF_E_SYMBOL;
      if (!inf_take(L, s, 2, rep)) return INF_E_INPUT;
      rep += 3;
      len = prev;
    } else if (sy == 17) {
      if (!inf_take(L, s, 3, rep)) return INF_E_INPUT;
      rep += 3;
    } else {
      if (!inf_take(L, s, 7, rep)) return INF_E_INPUT;
      rep += 11;
    }
    if (have + rep > hlit + hdist) return INF_E_SYMBOL;
    for (u32 k = FQ_LANE; k < rep; k += FQ_WAVE) ll[have + k] = (u8)len;
    prev = len;
    have += rep;
  }
  FQ_SYNC();
  if (uniform32(ll[256]) == 0) return INF_E_CODE;
  if ((err = inf_build(L, ll, hlit, INF_LENS, L.lcount, L.lsym, L.lfast))) return err;
  return inf_build(L, ll + hlit, hdist, INF_DISTS, L.dcount, L.dsym, L.dfast);
}

FQ_DEV u32 inf_fixed(InfLds &L) {
  u8 *ll = L.lens;
  for (u32 k = FQ_LANE; k < 320; k += FQ_WAVE) ll[k] = k < 144 ? 8 : k < 256 ? 9 : k < 280 ? 7 : k < 288 ? 8 : 5;
  FQ_SYNC();
  const u32 err = inf_build(L, ll, 288, INF_LENS, L.lcount, L.lsym, L.lfast);
  return err ? err : inf_build(L, ll + 288, 32, INF_DISTS, L.dcount, L.dsym, L.dfast);   // (30 and 31 have codes and are refused where they come up)
}

// a * b mod P, the CRC-32 polynomial, bit-reflected (x^0 is bit 31)
FQ_DEV u32 inf_crc_mul(u32 a, u32 b) {
  u32 p = 0;
  for (u32 m = 1u << 31; m; m >>= 1) {
    if (a & m) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ 0xedb88320u : b >> 1;
  }
  return p;
}
FQ_DEV u32 inf_crc_shift(u32 crc, u32 n_bytes) {   // crc * x^(8 n_bytes) mod P
  u32 q = 0x00800000u;   // x^8
  for (; n_bytes; n_bytes >>= 1) {
    if (n_bytes & 1u) crc = inf_crc_mul(crc, q);
    q = inf_crc_mul(q, q);
  }
  return crc;
}

// CRC-32 of w[0 .. n): slice i of INF_SLICES from the register value 0 (slice 0: ~0), shifted by the bytes behind it
FQ_DEV u32 inf_crc(InfLds &L, const u8 *w, u32 n) {
  u32 len = ((n + INF_SLICES - 1) / INF_SLICES + 3u) & ~3u;
  if (!((len >> 2) & 1u)) len += 4;   // (an odd number of words from slice to slice: the lanes read different banks)
  u32 acc = 0;
  for (u32 i = FQ_LANE; i < INF_SLICES; i += FQ_WAVE) {
    const u32 lo = inf_min32(i * len, n), hi = inf_min32(lo + len, n);
    u32 c = i ? 0u : ~0u;
    for (u32 p = lo; p < hi; ++p) c = L.crc_tab[(c ^ w[p]) & 0xffu] ^ (c >> 8);
    acc ^= inf_crc_shift(c, n - hi);
  }
  for (u32 o = FQ_WAVE / 2; o > 0; o >>= 1) acc ^= wave_xor32(acc, o);
  return ~acc;
}

FQ_DEV u32 inf_le32(const u8 *p) { return (u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24); }

// the member's deflate data into the window w; ends with s.op bytes there
FQ_DEV u32 inf_member(InfLds &L, InfState &s, u8 *w) {
  u32 err, last = 0;
  while (!last) {
    u32 type;
    if (!inf_take(L, s, 1, last) || !inf_take(L, s, 2, type)) return INF_E_INPUT;
    if (type == 3) return INF_E_BTYPE;
    if (type == 0) {
      u32 len, nlen;
      s.bits >>= s.nbits & 7u;
      s.nbits &= ~7u;
      if (!inf_take(L, s, 16, len) || !inf_take(L, s, 16, nlen)) return INF_E_INPUT;
      if ((len ^ 0xffffu) != nlen) return INF_E_STORED;
      const u64 pos = s.ip - s.nbits / 8;   // (what the bit buffer holds beyond the four bytes goes back)
      if (len > s.iend - pos) return INF_E_INPUT;
      if (len > s.out_len - s.op) return INF_E_OUTPUT;
      for (u32 k = FQ_LANE; k < len; k += FQ_WAVE) w[s.op + k] = s.in[pos + k];
      s.op += len;
      s.bits = 0;
      s.nbits = 0;
      s.ip = pos + len;
      inf_stage(L, s);
      continue;
    }
    if ((err = type == 1 ? inf_fixed(L) : inf_dynamic(L, s))) return err;
    for (;;) {
      u32 sy;
      if ((err = inf_symbol(L, s, L.lcount, L.lsym, L.lfast, sy))) return err;
      if (sy < 256) {
        if (s.op >= s.out_len) return INF_E_OUTPUT;
        if (FQ_LANE == 0) w[s.op] = (u8)sy;
        s.op += 1;
        continue;
      }
      if (sy == 256) break;
      if (sy > 285) return INF_E_SYMBOL;
      u32 x = inf_len_base(sy - 257), extra, ds;
      if (!inf_take(L, s, x >> 16, extra)) return INF_E_INPUT;
      const u32 len = (x & 0xffffu) + extra;
      if ((err = inf_symbol(L, s, L.dcount, L.dsym, L.dfast, ds))) return err;
      if (ds > 29) return INF_E_SYMBOL;
      x = inf_dist_base(ds);
      if (!inf_take(L, s, x >> 16, extra)) return INF_E_INPUT;
      const u32 d = (x & 0xffffu) + extra;
      if (d > s.op) return INF_E_DISTANCE;
      if (len > s.out_len - s.op) return INF_E_OUTPUT;
      // every source byte lies before the match: the literals and matches before it are in LDS, in order
      FQ_SYNC();
      const u8 *src = w + (s.op - d);
      for (u32 k = FQ_LANE; k < len; k += FQ_WAVE) w[s.op + k] = src[d > k ? k : k % d];
      s.op += len;
    }
  }
  FQ_SYNC();
  return INF_OK;
}

FQ_KERNEL64 void k_bgzf_inflate(InfCfg c) {
  FQ_SHARED InfLds L;
  const u32 m = FQ_BLOCK;
  if (m >= c.n) return;
  u32 err = INF_OK;
  const u64 lo = uniform64(c.in_off[m]), hi = uniform64(c.in_off[m + 1]);
  const u64 o_lo = uniform64(c.out_off[m]), o_hi = uniform64(c.out_off[m + 1]);
  InfState s;
  s.in = c.in;
  s.bits = 0; s.nbits = 0; s.op = 0;
  // header: 1f 8b 08, FLG with FEXTRA, XLEN at 10; the data ends 8 bytes before the member does
  if (hi < lo || hi - lo < 12 + 8 || o_hi < o_lo || o_hi - o_lo > INF_WINDOW || o_hi > c.out_cap) err = INF_E_HEADER;
  u32 xlen = 0;
  if (!err) {
    const u8 *h = c.in + lo;
    xlen = (u32)h[10] | ((u32)h[11] << 8);
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || (h[3] & 0x1eu) != 4u || 12ull + xlen + 8 > hi - lo) err = INF_E_HEADER;
  }
  if (!err) {
    s.ip = lo + 12 + xlen;
    s.iend = hi - 8;
    s.out_len = (u32)(o_hi - o_lo);
    u8 *w = (u8 *)L.win + ((o_lo + (u64)(uintptr_t)c.out) & 15u);
    for (u32 k = FQ_LANE; k < 256; k += FQ_WAVE) {
      u32 v = k;
      for (u32 b = 0; b < 8; ++b) v = (v & 1u) ? (v >> 1) ^ 0xedb88320u : v >> 1;
      L.crc_tab[k] = v;
    }
    inf_stage(L, s);
    err = inf_member(L, s, w);
    if (!err && (s.op != s.out_len || inf_le32(c.in + hi - 4) != s.out_len)) err = INF_E_ISIZE;
    if (!err && inf_crc(L, w, s.out_len) != inf_le32(c.in + hi - 8)) err = INF_E_CRC;
    if (!err) {
      u8 *dst = c.out + o_lo;
      const u32 n = s.out_len, head = inf_min32((16u - (u32)((uintptr_t)dst & 15u)) & 15u, n), body = (n - head) & ~15u;
      for (u32 k = FQ_LANE; k < head; k += FQ_WAVE) dst[k] = w[k];
      for (u32 k = FQ_LANE; k < body / 16; k += FQ_WAVE) *(Inf16 *)(dst + head + 16ull * k) = *(const Inf16 *)(w + head + 16u * k);
      for (u32 k = head + body + FQ_LANE; k < n; k += FQ_WAVE) dst[k] = w[k];
    }
  }
  if (FQ_LANE == 0) c.status[m] = err;
}
