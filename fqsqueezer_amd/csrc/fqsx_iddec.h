// fqsx_iddec.h -- read-id stream decoder on the GPU: the inverse of id_encode_body (fqsx_idk.h), following the reference's
// decoder (CIdCompressor::Decompress / DecompressPE, id.cpp:182-228; decompress_lossless :495-666; decompress_instrument
// :669-731; ResetReadPrev :124-135; tokenize :734-757; store_int, id.h:117-149; mtf.cpp).  Same shape as the encoder: one
// wavefront per logical worker, the same worker partition and the same model tables (IdCfg small / big / fixed / mtf, q_hash,
// find-or-claim), so that k_qual_rehash, k_id_init_fixed and the IDM_* keys serve both directions.  The control flow is
// wave-uniform and the coder state (QDec, fqsx_qdec.h) scalar; the lanes work inside one symbol: lane l holds statistics
// 4l .. 4l + 3 of a 128- / 256-symbol model (one u64 of the slot), the symbol search is an in-lane prefix, one wave scan and a
// ballot.  The 2- and 4-symbol models are a scalar job.  The line being decoded, the previous one, the two token sets and the
// deltas live in LDS (IdShared).  What comes back is what the reference's decoder writes, not what its encoder was given: a
// numeric token is rebuilt by store_int from previous value + delta (leading zeros are lost), and the decoder tokenises what
// it wrote.  Included by fqsx_api.hip after fqsx_idk.h and fqsx_qdec.h.
#pragma once
#include "fqsx_idk.h"
#include "fqsx_qdec.h"

enum { IDK_ERR_STREAM = 7 /* cumulative frequency at or above the total, impossible move-to-front code, reading beyond the stream */ };

struct IdDecArgs {
  const u8 *in;        // the T streams back to back, every start 8-byte aligned, zero padded to whole words
  const u64 *in_off;   // [T] start of worker w's stream inside `in`, then [T] its length in bytes
  u32 *id_len;         // [n_reads] bytes of every decoded id line (with its line feed)
};
// Output: worker w writes its lines back to back into cfg.out + w * cfg.out_cap and their total into cfg.lens[w].
// *cfg.err = error | which << 8; which: the capacity IDK_ERR_TABLE ran out of (1 small, 2 big).

struct IdD {
  const IdCfg *cfg;
  IdShared *sm;
  QDec d;
  u64 *small, *big, *fixed;
  u8 *mtf;
  u32 n_small, n_big, n_mtf;
  u32 cur_set;             // which token set receives the line being decoded (the other: the previous line's)
  u32 n_tok0, n_tok1;      // tokens in set 0 / 1 (two scalars, not an array: an index that is not a constant would keep the whole state in scratch)
  u64 ctx_flags, ctx_pe_flags;
  u32 err, which;
  u8 *out;
  u64 out_pos;
};

FQ_DEV u32 idd_n_tok(const IdD &k, u32 set) { return set ? k.n_tok1 : k.n_tok0; }

// ---- models -----------------------------------------------------------------------------------------------------------
// small model of `map` at context `ctx`: decode one symbol
FQ_DEV u32 idd_small(IdD &k, u32 map, u64 ctx, u32 N) {
  bool fresh;
  u64 *slot = idw_small_slot(k, map, ctx, fresh);
  if (!slot) { k.which = 1; return 0; }
  const u64 st = idm_small_load(slot, N, fresh);
  u32 tot = 0;
  for (u32 i = 0; i < N; ++i) tot += idm_field(st, i);
  const u32 cumv = qd_cum(k.d, tot);
  if (cumv >= tot) { k.err = IDK_ERR_STREAM; return 0; }
  u32 x = 0, cum = 0;
  for (; x + 1 < N; ++x) {
    if (cum + idm_field(st, x) > cumv) break;
    cum += idm_field(st, x);
  }
  qd_update(k.d, idm_field(st, x), cum);
  idm_small_update_store(slot, st, N, x, tot);
  return x;
}
// N-symbol model (N <= 256) in a big slot: decode one symbol.  Four statistics per lane.
FQ_DEV u32 idd_big_decode(IdD &k, u64 *slot, u32 N, bool fresh) {
  u64 *w = slot + 1;
#if FQ_WAVE > 1
  const u32 l = FQ_LANE;
  u64 v = fresh ? 0x0001000100010001ULL : w[l];   // (a new model: all ones, entries beyond N are never read)
  u32 tot = fresh ? N : (u32)uniform64(w[64]);
  const u32 s0 = 4 * l < N ? (u32)(v & 0xffff) : 0, s1 = 4 * l + 1 < N ? (u32)((v >> 16) & 0xffff) : 0;
  const u32 s2 = 4 * l + 2 < N ? (u32)((v >> 32) & 0xffff) : 0, s3 = 4 * l + 3 < N ? (u32)(v >> 48) : 0;
  const u32 p1 = s0, p2 = p1 + s1, p3 = p2 + s2, t = p3 + s3;
  const u32 ex = wave_excl_scan32(t);
  const u32 cumv = qd_cum(k.d, tot);
  const u64 b = wave_ballot(ex + t > cumv);
  if (!b) { k.err = IDK_ERR_STREAM; return 0; }
  const u32 L = uniform32(ctz64(b));
  const u32 c = cumv - ex;   // (meaningful in lane L: 0 <= c < t)
  const u32 f = (c >= p1 ? 1u : 0u) + (c >= p2 ? 1u : 0u) + (c >= p3 ? 1u : 0u);
  const u32 fL = qd_rl(f, L);
  const u32 freq = qd_rl(f == 0 ? s0 : f == 1 ? s1 : f == 2 ? s2 : s3, L);
  const u32 cum = qd_rl(ex + (f == 0 ? 0u : f == 1 ? p1 : f == 2 ? p2 : p3), L);
  const u32 sym = 4 * L + fL;
  qd_update(k.d, freq, cum);
  // Update (rc.h:41-55): the symbol's statistic and the total, everything halved while the total reaches 2^15
  if (l == L) v += 1ull << (16 * fL);
  tot += 1;
  bool all = fresh;
  while (tot >= (1u << 15)) {
    u32 part = 0;
    v = idm_halve_word(v, 4 * l, N, part);
    tot = uniform32(wave_sum32(part));
    all = true;
  }
  if (all || l == L) w[l] = v;
  if (l == 0) w[64] = tot;
  FQ_SYNC_MEM();
  return sym;
#else
  if (fresh) {
    for (u32 i = 0; i < 64; ++i) w[i] = 0x0001000100010001ULL;
    w[64] = N;
  }
  u32 tot = (u32)w[64];
  const u32 cumv = qd_cum(k.d, tot);
  if (cumv >= tot) { k.err = IDK_ERR_STREAM; return 0; }
  u32 x = 0, cum = 0;
  for (; x + 1 < N; ++x) {
    const u32 f = (u32)((w[x >> 2] >> (16 * (x & 3))) & 0xffff);
    if (cum + f > cumv) break;
    cum += f;
  }
  qd_update(k.d, (u32)((w[x >> 2] >> (16 * (x & 3))) & 0xffff), cum);
  w[x >> 2] += 1ull << (16 * (x & 3));
  tot += 1;
  while (tot >= (1u << 15)) {
    tot = 0;
    for (u32 i = 0; 4 * i < N; ++i) w[i] = idm_halve_word(w[i], 4 * i, N, tot);
  }
  w[64] = tot;
  return x;
#endif
}
FQ_DEV u32 idd_big(IdD &k, u32 map, u64 ctx, u32 N) {
  bool fresh;
  u64 *slot = idw_big_slot(k, map, ctx, fresh);
  if (!slot) { k.which = 2; return 0; }
  return idd_big_decode(k, slot, N, fresh);
}
FQ_DEV u32 idd_fixed(IdD &k, u32 which, u32 N) { return idd_big_decode(k, k.fixed + IDK_BIG_U64 * which, N, false); }

// ---- the line in sm->cur ------------------------------------------------------------------------------------------------
FQ_DEV void idd_put(IdD &k, u32 &size, u8 c) {
  if (size >= IDK_MAX_ID) { k.err = IDK_ERR_TOO_LONG; return; }
  if (FQ_LANE == 0) k.sm->cur[size] = c;
  ++size;
}
// store_int, id.h:117-149: 1 digit below 10 (also for negative values, whose "digit" is '0' + val % 10), none from 10^15
FQ_DEV void idd_store_int(IdD &k, u32 &size, long long val) {
  u32 n_dig = 0;
  if (val < 1000000000000000ll) {
    n_dig = 1;
    for (long long t = 10; n_dig < 15 && val >= t; t *= 10) ++n_dig;
  }
  if (size + n_dig > IDK_MAX_ID) { k.err = IDK_ERR_TOO_LONG; return; }
  for (u32 i = n_dig; i-- > 0;) {
    if (FQ_LANE == 0) k.sm->cur[size + i] = (u8)('0' + (int)(val % 10));
    val /= 10;
  }
  size += n_dig;
}
// tokenize (id.cpp:734-757) of sm->cur[0, size) into token set `set`
FQ_DEV void idd_tokenize(IdD &k, u32 size, u32 set) {
  IdShared *sm = k.sm;
  FQ_SYNC();
  for (u32 i = FQ_LANE; i < size; i += FQ_WAVE) {
    const u8 c = sm->cur[i];
    sm->cls[i] = idk_is_num(c) ? 0 : idk_is_lit(c) ? 1 : 2;
  }
  FQ_SYNC();
  u32 n_tok = 0, start = 0;
  bool numeric = true;
  for (u32 i = 0; i < size; ++i) {
    const u32 c = sm->cls[i];
    if (c == 2) {
      if (numeric && (i - start >= 11 || i == start)) numeric = false;
      if (n_tok >= IDK_MAX_TOK) { k.err = IDK_ERR_TOO_LONG; return; }
      if (FQ_LANE == 0) { sm->tb[set][n_tok] = (u16)start; sm->te[set][n_tok] = (u16)i; sm->tn[set][n_tok] = numeric ? 1 : 0; sm->ts[set][n_tok] = sm->cur[i]; }
      ++n_tok;
      numeric = true;
      start = i + 1;
    } else if (c == 1)
      numeric = false;
  }
  FQ_SYNC();
  if (set) k.n_tok1 = n_tok; else k.n_tok0 = n_tok;
}
// decompress_lossless, id.cpp:495-666: one line into sm->cur; returns its size.  The line then is the previous one.
FQ_DEV u32 idd_lossless(IdD &k) {
  IdShared *sm = k.sm;
  const u32 cs = k.cur_set, ps = cs ^ 1u;
  u32 size = 0;
  const u8 *q = sm->prev;
  if (idd_small(k, IDM_FLAGS, k.ctx_flags, 2) == 1 && !k.err) {   // tokens of the same types as the previous line's
    k.ctx_flags = ((k.ctx_flags << 1) + 1) & 0xff;
    const u32 n_tok = idd_n_tok(k, ps);
    for (u32 i = 0; i < n_tok && !k.err; ++i) {
      const u32 pb = sm->tb[ps][i], pe = sm->te[ps][i], len = pe - pb;
      if (!sm->tn[ps][i]) {
        if (idd_small(k, IDM_LIT_SAME, i, 2) == 1) {           // the same token
          if (k.err) break;
          if (size + len > IDK_MAX_ID) { k.err = IDK_ERR_TOO_LONG; break; }
          for (u32 j = FQ_LANE; j < len; j += FQ_WAVE) sm->cur[size + j] = q[pb + j];
          size += len;
        } else if (k.err) {
          break;
        } else if (idd_small(k, IDM_LIT_SAME_LEN, i, 2) == 1) {   // the same length: 0 = the previous line's byte
          for (u32 j = 0; j < len && !k.err; ++j) {
            const u32 d = idd_big(k, IDM_LITERAL, k.ctx_flags + (1ull << 32) + j, 128);
            if (!k.err) idd_put(k, size, d == 0 ? q[pb + j] : (u8)d);
          }
        } else {                                                // bytes up to a 0
          for (u32 j = 0; !k.err; ++j) {
            const u32 d = idd_big(k, IDM_LITERAL, k.ctx_flags + j, 128);
            if (k.err || d == 0) break;
            idd_put(k, size, (u8)d);
          }
        }
      } else {
        const long long v_prev = idk_get_int(q, pb, pe), d0 = sm->deltas[i];
        u64 ctx = (u64)i << 40;
        ctx += idk_ilog2(d0 < 0 ? 0ull - (u64)d0 : (u64)d0) << 31;
        ctx += (u64)(d0 < 0) << 30;
        long long delta;
        u32 d = idd_small(k, IDM_NUM_SMALL, ctx, 4);
        if (k.err) break;
        if (d < 3)
          delta = (long long)d - 1;
        else {
          u32 n_bytes = 0;
          u64 ud = 0;
          d = idd_big(k, IDM_NUM_SIZE, ctx, 256);
          if (k.err) break;
          if (d <= 246) ud = (u64)((long long)d - 123);
          else if (d == 247) { n_bytes = 2; ctx += 0x10; }
          else if (d == 248) { n_bytes = 3; ctx += 0x20; }
          else if (d == 249) { n_bytes = 4; ctx += 0x30; }
          else if (d == 250) { n_bytes = 8; ctx += 0x40; }
          else if (d == 251) { n_bytes = 2; ctx += 0x50; }
          else if (d == 252) { n_bytes = 3; ctx += 0x60; }
          else if (d == 253) { n_bytes = 4; ctx += 0x70; }
          else if (d == 254) { n_bytes = 8; ctx += 0x80; }
          for (u32 j = 0; j < n_bytes && !k.err; ++j) ud += (u64)idd_big(k, IDM_NUM_SIZE, ctx + j, 256) << (8 * j);
          if (k.err) break;
          if (d >= 251) ud = 0ull - ud;
          delta = (long long)ud;
        }
        FQ_SYNC();
        if (FQ_LANE == 0) sm->deltas[i] = delta;
        FQ_SYNC();
        idd_store_int(k, size, (long long)((u64)delta + (u64)v_prev));
      }
      if (!k.err) idd_put(k, size, sm->ts[ps][i]);
    }
    if (k.err) return 0;
    idd_tokenize(k, size, cs);
  } else {
    if (k.err) return 0;
    k.ctx_flags = (k.ctx_flags << 1) & 0xff;
    for (u32 i = 0; !k.err; ++i) {   // the plain line ends at a line feed or -- the instrument name -- at a 0
      const u32 c = idd_big(k, IDM_PLAIN, i, 128);
      if (k.err) break;
      idd_put(k, size, (u8)c);
      if (c == 0 || c == 0x0A) break;
    }
    if (k.err) return 0;
    idd_tokenize(k, size, cs);
    FQ_SYNC();
    for (u32 i = FQ_LANE; i < idd_n_tok(k, cs); i += FQ_WAVE) sm->deltas[i] = 0;
    FQ_SYNC();
  }
  if (k.err) return 0;
  FQ_SYNC();
  for (u32 i = FQ_LANE; i < size; i += FQ_WAVE) sm->prev[i] = sm->cur[i];
  FQ_SYNC();
  k.cur_set = ps;
  return size;
}
// the line sm->cur[0, size) is the id of read `read`
FQ_DEV void idd_emit(IdD &k, const IdDecArgs &da, u64 read, u32 size) {
  if (k.err) return;
  if (k.out_pos + size > k.cfg->out_cap) { k.err = IDK_ERR_OUT; return; }
  FQ_SYNC();
  for (u32 i = FQ_LANE; i < size; i += FQ_WAVE) k.out[k.out_pos + i] = k.sm->cur[i];
  if (FQ_LANE == 0) da.id_len[read] = size;
  k.out_pos += size;
}
// sm->name (length byte + bytes) goes to the front of the move-to-front list, the entries [0, pos) one place down
FQ_DEV void idd_mtf_front(IdD &k, u32 pos) {
  IdShared *sm = k.sm;
  const u32 nl = sm->name[0];
  FQ_SYNC_MEM();
  for (u32 e = pos; e > 0; --e) {
    u64 *d = (u64 *)(k.mtf + (u64)e * IDK_NAME);
    const u64 *s = (const u64 *)(k.mtf + (u64)(e - 1) * IDK_NAME);
    for (u32 l = FQ_LANE; l < IDK_NAME / 8; l += FQ_WAVE) d[l] = s[l];
    FQ_SYNC_MEM();
  }
  for (u32 j = FQ_LANE; j < IDK_NAME; j += FQ_WAVE) k.mtf[j] = j <= nl ? sm->name[j] : 0;
  FQ_SYNC_MEM();
}
// decompress_instrument, id.cpp:669-731: the instrument name and a line feed
FQ_DEV u32 idd_instrument(IdD &k) {
  IdShared *sm = k.sm;
  const u32 flag = idd_fixed(k, 0, 11);
  if (k.err) return 0;
  if (flag == 0) {   // a new name: through the lossless path with its terminating 0, which becomes the line feed
    const u32 size = idd_lossless(k);
    if (k.err) return 0;
    if (size == 0) { k.err = IDK_ERR_STREAM; return 0; }
    FQ_SYNC();
    u32 nl = 0;
    while (nl < size && sm->cur[nl] != 0) ++nl;   // std::string(char*): the bytes up to the first 0
    if (nl + 1 > IDK_NAME - 1) { k.err = IDK_ERR_TOO_LONG; return 0; }
    if (k.n_mtf >= k.cfg->mtf_cap) { k.err = IDK_ERR_MTF_FULL; return 0; }
    for (u32 j = FQ_LANE; j < nl; j += FQ_WAVE) sm->name[1 + j] = sm->cur[j];
    if (FQ_LANE == 0) { sm->name[0] = (u8)nl; sm->cur[size - 1] = '\n'; }
    FQ_SYNC();
    idd_mtf_front(k, k.n_mtf);
    k.n_mtf += 1;
    return size;
  }
  u32 code;
  if (flag < 3) code = flag - 1;
  else if (flag < 10) code = idd_fixed(k, flag - 2, 2u << (flag - 3)) + (2u << (flag - 3));
  else {
    code = 0;
    for (u32 i = 0; i < 4 && !k.err; ++i) code += idd_fixed(k, 8 + i, 256) << (8 * i);
  }
  if (k.err) return 0;
  if (code >= k.n_mtf) { k.err = IDK_ERR_STREAM; return 0; }
  // mtf.Insert(code), then entry 0
  FQ_SYNC();
  for (u32 j = FQ_LANE; j < IDK_NAME; j += FQ_WAVE) sm->name[j] = k.mtf[(u64)code * IDK_NAME + j];
  FQ_SYNC_MEM();
  const u32 nl = sm->name[0];
  if (nl + 1 > IDK_NAME - 1) { k.err = IDK_ERR_STREAM; return 0; }
  if (code > 0) idd_mtf_front(k, code);
  for (u32 j = FQ_LANE; j < nl; j += FQ_WAVE) sm->cur[j] = sm->name[1 + j];
  if (FQ_LANE == 0) sm->cur[nl] = '\n';
  FQ_SYNC();
  return nl + 1;
}

// worker `tid` decodes the ids of its reads of the block (CIdCompressor::Decompress / DecompressPE, application.cpp:874-917)
FQ_DEV void id_decode_body(const IdCfg &cfg, const IdDecArgs &da, IdShared *sm, u32 tid, u32 n_reads, u32 paired) {
  const u64 T = cfg.T;
  u64 first, last;
  worker_reads(tid, T, n_reads, first, last);
  IdD k;
  idw_open(k, cfg, sm, tid);
  k.d.in = da.in + uniform64(da.in_off[tid]);
  k.d.len = uniform64(da.in_off[T + tid]);
  qd_start(k.d);
  k.n_tok0 = k.n_tok1 = 0;
  k.which = 0;
  k.out = cfg.out + (u64)tid * cfg.out_cap;
  k.out_pos = 0;
  for (u64 i = first; i < last && !k.err; i += paired ? 2 : 1) {
    if (!paired) {
      const u32 size = cfg.mode == 0 ? idd_lossless(k) : idd_instrument(k);
      idd_emit(k, da, i, size);
      continue;
    }
    if (cfg.mode == 0) {   // DecompressPE, id.cpp:195-228
      const u32 typical = idd_small(k, IDM_PE_FLAGS, k.ctx_pe_flags, 2);
      if (k.err) break;
      k.ctx_pe_flags = ((k.ctx_pe_flags << 1) + typical) & 0xff;
      u32 size = idd_lossless(k);
      idd_emit(k, da, i, size);
      if (k.err) break;
      if (typical) {   // mate 2: a copy of mate 1 with the byte before the line feed set to '2' (the previous id stays mate 1's)
        FQ_SYNC();
        if (FQ_LANE == 0 && size >= 2) sm->cur[size - 2] = '2';
        FQ_SYNC();
      } else
        size = idd_lossless(k);
      idd_emit(k, da, i + 1, size);
    } else {
      u32 size = idd_instrument(k);
      idd_emit(k, da, i, size);
      if (k.err) break;
      size = idd_instrument(k);
      idd_emit(k, da, i + 1, size);
    }
  }
  if (!k.err && k.d.pos > k.d.len) k.err = IDK_ERR_STREAM;   // (a decoder consumes exactly the bytes the encoder wrote: this stream was cut short)
  if (FQ_LANE == 0) {
    cfg.lens[tid] = k.out_pos;
    idw_store_counts(k, tid);
    if (k.err) *cfg.err = k.err | (k.which << 8);
  }
}
