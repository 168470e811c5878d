// fqsx_qdec.h -- quality stream decoder on the GPU (CQualityCompressor::Decompress, quality.cpp:175-200;
// CRangeCoderModel::Decode, rc.h:403-421; CRangeDecoder, sub_rc.h:93-158).  Same shape as the encoder in fqsx_qual.h: one
// wavefront per logical worker and the same per-worker context table (QualCfg, q_hash, find-or-claim), so that k_qual_rehash
// and the host's sizing rule serve both.  The context of position i + 1 contains the symbol decoded at position i, so the
// positions of a read are strictly sequential and the 64 lanes work inside one position: lane l holds the statistics of
// symbols l and l + 64 of the current model, the symbol search is one wave prefix sum and a ballot, the halving one step
// per lane.  The coder state is wave-uniform.  In the modes of 2 / 4 / 8 symbols the lanes look up the home slots of the
// n_sym possible contexts of the next position (read-only) while a position is decoded, which takes the dependent table
// round trip out of the per-symbol chain.  Included by fqsx_api.hip after fqsx_qual.h.
#pragma once
#include "fqsx_qual.h"

struct QualDecArgs {
  const u8 *in;        // the T streams back to back, every start 8-byte aligned, zero padded to whole words
  const u64 *in_off;   // [T] start of worker w's stream inside `in`, then [T] its length in bytes
  u8 *out;             // the block's qualities (ASCII), addressed by cfg.off
  u8 rev[96];          // quality_code_map_rev
};

// CRangeDecoder (fqsx_rc.h) on wave-uniform state.  The stream is read as aligned 8-byte words, one word ahead of its use;
// bytes at and beyond `len` read as 0 and words that lie wholly beyond it are not loaded.
struct QDec { RcDec rc; u64 pos, len, cur, nxt; const u8 *in; };
FQ_DEV u64 qd_word(const QDec &d, u64 p) {   // the word holding bytes [p, p + 8), p a multiple of 8
  if (p >= d.len) return 0;
  u64 v = uniform64(*(const u64 *)(d.in + p));
  const u64 left = d.len - p;
  if (left < 8) v &= (1ull << (8 * (u32)left)) - 1ull;
  return v;
}
FQ_DEV u64 rc_src_byte(QDec &d) {
  const u64 b = (d.cur >> (8 * (u32)(d.pos & 7))) & 0xff;
  ++d.pos;
  if ((d.pos & 7) == 0) { d.cur = d.nxt; d.nxt = qd_word(d, d.pos + 8); }
  return b;
}
FQ_DEV void qd_start(QDec &d) {
  d.pos = 0;
  d.cur = qd_word(d, 0);
  d.nxt = qd_word(d, 8);
  rcd_start(d.rc, d, d.len);
}
FQ_DEV u32 qd_cum(QDec &d, u32 tot) { return uniform32(rcd_cum(d.rc, tot)); }
FQ_DEV void qd_update(QDec &d, u32 freq, u32 cum) { rcd_update(d.rc, d, freq, cum); }

// The model of the current context in registers: N statistics and their total (the slot's packed u16 fields 0..N)
#if FQ_WAVE > 1
struct QModel { u32 s0, s1, tot; };   // s0 / s1 = statistics of symbols lane / lane + 64 (0 beyond the alphabet)
FQ_DEV u32 qd_rl(u32 v, u32 lane) { return (u32)__builtin_amdgcn_readlane((int)v, (int)lane); }
FQ_DEV u64 qd_rl64(u64 v, u32 lane) { return ((u64)qd_rl((u32)(v >> 32), lane) << 32) | qd_rl((u32)v, lane); }
FQ_DEV void qm_from_fields(QModel &m, u32 N, u32 f0, u32 f1) {   // f0 / f1 = fields lane / lane + 64 (the total is field N)
  m.tot = qd_rl(N < 64 ? f0 : f1, N & 63);
  m.s0 = FQ_LANE < N ? f0 : 0;
  m.s1 = FQ_LANE + 64 < N ? f1 : 0;
}
FQ_DEV void qm_load(QModel &m, u32 N, const u64 *slot) {   // one round trip: the slot is contiguous
  const u16 *f = (const u16 *)(slot + 1);
  const u32 f0 = FQ_LANE <= N ? f[FQ_LANE] : 0, f1 = FQ_LANE + 64 <= N ? f[FQ_LANE + 64] : 0;
  qm_from_fields(m, N, f0, f1);
}
FQ_DEV void qm_fresh(QModel &m, u32 N) {   // new model: all 1, total N (rc.h:69-74)
  m.s0 = FQ_LANE < N ? 1 : 0;
  m.s1 = FQ_LANE + 64 < N ? 1 : 0;
  m.tot = N;
}
// GetSym (rc.h:129-141) + GetFreq: the first symbol whose running sum exceeds cumv.  Both halves of the alphabet go through
// one scan, packed 16 + 16 bits (every partial sum is at most the total, which is below 2^15).  False: cumv >= total.
FQ_DEV bool qm_search(const QModel &m, u32 N, u32 cumv, u32 &sym, u32 &freq, u32 &cum) {
  const u32 pk = m.s0 | (m.s1 << 16), ex = wave_excl_scan32(pk);
  const u32 sum0 = (qd_rl(ex, 63) + qd_rl(pk, 63)) & 0xffff;
  const u32 e0 = ex & 0xffff, e1 = sum0 + (ex >> 16);
  const u64 b0 = wave_ballot(e0 + m.s0 > cumv);
  if (b0) {
    const u32 l = uniform32(ctz64(b0));
    sym = l; freq = qd_rl(m.s0, l); cum = qd_rl(e0, l);
    return true;
  }
  const u64 b1 = wave_ballot(e1 + m.s1 > cumv);
  if (b1) {
    const u32 l = uniform32(ctz64(b1));
    sym = 64 + l; freq = qd_rl(m.s1, l); cum = qd_rl(e1, l);
    return true;
  }
  sym = N - 1;   // (malformed stream) the last symbol
  freq = N > 64 ? qd_rl(m.s1, (N - 1) & 63) : qd_rl(m.s0, N - 1);
  cum = m.tot - freq;
  return false;
}
// Update (rc.h:120-127) and the model's way back into its slot: the symbol's statistic and the total, or -- new model,
// halving at 2^15 (one halving always suffices, see qual_chunk) -- every field
FQ_DEV void qm_update_store(QModel &m, u32 N, u32 sym, u64 *slot, bool fresh) {
  u16 *f = (u16 *)(slot + 1);
  if (FQ_LANE == (sym & 63)) { if (sym < 64) m.s0 += 1; else m.s1 += 1; }
  u32 ntot = m.tot + 1;
  const bool halve = ntot >= (1u << 15);
  if (halve) {
    m.s0 = (m.s0 + 1) >> 1;
    m.s1 = (m.s1 + 1) >> 1;
    ntot = uniform32(wave_sum32(m.s0 + m.s1));
  }
  if (halve || fresh) {
    if (FQ_LANE < N) f[FQ_LANE] = (u16)m.s0;
    if (FQ_LANE + 64 < N) f[FQ_LANE + 64] = (u16)m.s1;
  } else if (FQ_LANE == (sym & 63)) {
    f[sym] = (u16)(sym < 64 ? m.s0 : m.s1);
  }
  if (FQ_LANE == 0) f[N] = (u16)ntot;
  m.tot = ntot;
}
#else
struct QModel { u32 st[96], tot; };
FQ_DEV void qm_load(QModel &m, u32 N, const u64 *slot) {
  const u16 *f = (const u16 *)(slot + 1);
  for (u32 i = 0; i < N; ++i) m.st[i] = f[i];
  m.tot = f[N];
}
FQ_DEV void qm_fresh(QModel &m, u32 N) {
  for (u32 i = 0; i < N; ++i) m.st[i] = 1;
  m.tot = N;
}
FQ_DEV bool qm_search(const QModel &m, u32 N, u32 cumv, u32 &sym, u32 &freq, u32 &cum) {
  u32 t = 0;
  for (u32 i = 0; i < N; ++i) {
    if (t + m.st[i] > cumv) { sym = i; freq = m.st[i]; cum = t; return true; }
    t += m.st[i];
  }
  sym = N - 1; freq = m.st[N - 1]; cum = m.tot - freq;
  return false;
}
FQ_DEV void qm_update_store(QModel &m, u32 N, u32 sym, u64 *slot, bool fresh) {
  u16 *f = (u16 *)(slot + 1);
  m.st[sym] += 1;
  u32 ntot = m.tot + 1;
  const bool halve = ntot >= (1u << 15);
  if (halve) {
    ntot = 0;
    for (u32 i = 0; i < N; ++i) { m.st[i] = (m.st[i] + 1) >> 1; ntot += m.st[i]; }
  }
  if (halve || fresh) { for (u32 i = 0; i < N; ++i) f[i] = (u16)m.st[i]; } else f[sym] = (u16)m.st[sym];
  f[N] = (u16)ntot;
  m.tot = ntot;
}
#endif

// The home slots of the possible contexts of the next position, looked at while the current one is decoded.  Read-only:
// only the context of the symbol that is decoded may be claimed (a claimed slot whose model is never written would later
// pass for an existing one, and `filled` has to end equal to the encoder's).
struct QAhead {
#if FQ_WAVE > 1
  u64 k;           // key found in the home slot of candidate `lane`
  u64 w[3];        // ... and the slot's statistics words
#else
  u64 k[8];
#endif
};
// (the modes of 2 / 4 / 8 symbols only: with the 96 candidates of the lossless mode the look-ups cost more than they save,
// profiles/qual_decode.json, so that mode takes the plain look-up once the symbol is known)
FQ_DEV bool qd_looks_ahead(const QualCfg &cfg) {
#ifndef FQSX_QDEC_NO_LOOKAHEAD
  return cfg.n_sym <= 8;
#else
  return false;
#endif
}
FQ_DEV void qd_look_ahead(const QualCfg &cfg, const u64 *tab, u64 pos_next, u64 hist, QAhead &a) {
  const u32 N = cfg.n_sym;
#if FQ_WAVE > 1
  a.k = 0; a.w[0] = a.w[1] = a.w[2] = 0;
  if (FQ_LANE < N) {
    const u64 ctx = (pos_next << 48) + (((hist << cfg.bits) + FQ_LANE) & cfg.ctx_mask);
    const u64 *p = tab + (q_hash(ctx) & cfg.cap_mask) * cfg.slot_u64;
    a.k = p[0];
#pragma unroll
    for (u32 j = 0; j < 3; ++j) if (j + 2 <= cfg.slot_u64) a.w[j] = p[1 + j];
  }
#else
  for (u32 c = 0; c < N; ++c) {
    const u64 ctx = (pos_next << 48) + (((hist << cfg.bits) + c) & cfg.ctx_mask);
    a.k[c] = tab[(q_hash(ctx) & cfg.cap_mask) * cfg.slot_u64];
  }
#endif
}
// The model of context `ctx` (= the candidate of symbol `sym`): from the look-ahead if its home slot settled the search,
// else the plain look-up from where the look-ahead stopped
FQ_DEV u64 *qd_open(const QualCfg &cfg, u64 *tab, u64 ctx, u32 sym, const QAhead &a, bool ahead, QModel &m, bool &fresh) {
  const u32 N = cfg.n_sym;
  u64 h = q_hash(ctx) & cfg.cap_mask, it0 = 0;
  u64 *slot = nullptr;
  bool have_model = false;
  fresh = false;
  if (ahead) {
#if FQ_WAVE > 1
    const u64 k = qd_rl64(a.k, sym);
#else
    const u64 k = a.k[sym];
#endif
    u64 *p = tab + h * cfg.slot_u64;
    if (k == ctx) {
      slot = p;
#if FQ_WAVE > 1
      // the statistics came with the key: fields 0..N of the broadcast words, one per lane
      const u64 w0 = qd_rl64(a.w[0], sym), w1 = qd_rl64(a.w[1], sym), w2 = qd_rl64(a.w[2], sym);
      const u32 wi = FQ_LANE >> 2;
      const u64 wv = wi == 0 ? w0 : wi == 1 ? w1 : w2;
      qm_from_fields(m, N, FQ_LANE <= N ? (u32)((wv >> (16 * (FQ_LANE & 3))) & 0xffff) : 0, 0);
      have_model = true;
#endif
    } else if (k == ~0ull) {
      if (FQ_LANE == 0) p[0] = ctx;
      slot = p;
      fresh = true;
    } else {
      h = (h + 1) & cfg.cap_mask;
      it0 = 1;
    }
  }
  // find_rc_context (quality.cpp:218-226) from probe it0: claimed if the sequence ends at an empty slot (the host sizes the table)
  if (!slot) slot = q_find<false>(tab, cfg.cap_mask, cfg.slot_u64, ctx, h, it0, true, fresh);
  if (!slot) return nullptr;
  if (fresh) {
    qm_fresh(m, N);
    FQ_SYNC_MEM();   // the claim is in memory before the next look-ahead reads home slots (one of them may be this slot)
  } else if (!have_model)
    qm_load(m, N, slot);
  return slot;
}

// 64 decoded symbols wait in the lanes (lane = output address & 63) and leave as aligned 8-byte words; the words the
// worker's range [lo, hi) covers only in part leave byte by byte (the neighbours belong to other workers)
FQ_DEV void qd_flush(u8 *out, u64 base, u64 lo, u64 hi, u32 byte) {
#if FQ_WAVE > 1
  u64 v = (u64)byte << (8 * (FQ_LANE & 7));
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) v |= __shfl_xor(v, o, 64);
  const u64 a = base + FQ_LANE, w0 = a & ~7ull;
  if (w0 >= lo && w0 + 8 <= hi) {
    if ((FQ_LANE & 7) == 0) *(u64 *)(out + w0) = v;
  } else if (a >= lo && a < hi)
    out[a] = (u8)byte;
#endif
}

// worker `tid` decodes the qualities of its reads of the block (application.cpp:874-917, quality.cpp:175-200)
FQ_DEV void qual_decode_body(const QualCfg &cfg, const QualDecArgs &da, u32 tid, u32 n_reads) {
  const u64 T = cfg.T;
  u64 first, last;
  worker_reads(tid, T, n_reads, first, last);
  const u32 N = cfg.n_sym;
  QDec d;
  d.in = da.in + uniform64(da.in_off[tid]);
  d.len = uniform64(da.in_off[T + tid]);
  qd_start(d);
  u64 *tab = cfg.tab + (u64)tid * (cfg.cap_mask + 1) * cfg.slot_u64;
  u32 filled = cfg.filled[tid], err = 0;
  const u64 o_lo = uniform64(cfg.off[first]), o_hi = uniform64(cfg.off[last]);   // the worker's output range
  u64 op = o_lo;       // next output address
#if FQ_WAVE > 1
  u32 obyte = 0;       // this lane's byte of the 64 addresses around op
#endif
  QModel m;
  QAhead ah;
  const bool la = qd_looks_ahead(cfg);
  for (u64 r = first; r < last && !err; ++r) {
    const u64 r0 = uniform64(cfg.off[r]), r1 = uniform64(cfg.off[r + 1]);
    if (r0 != op || r1 < r0 || r1 > o_hi) { err = 4; break; }   // (offsets that do not ascend: the host checks them)
    const u64 size = r1 - r0;
    if (size == 0) continue;
    u64 hist = cfg.ctx_mask;   // reset_context, quality.cpp:204-206
    bool fresh;
    u64 *slot = qd_open(cfg, tab, hist, 0, ah, false, m, fresh);
    for (u64 i = 0; i < size; ++i) {
      if (!slot) { err = 2; break; }
      if (fresh && (u64)(++filled) * 10 >= (cfg.cap_mask + 1) * 9) { err = 2; break; }
      if (la && i + 1 < size) qd_look_ahead(cfg, tab, i + 1, hist, ah);
      u32 sym, freq, cum;
      if (!qm_search(m, N, qd_cum(d, m.tot), sym, freq, cum)) err = 3;   // (goes on with the clamped symbol: everything stays in bounds)
      qd_update(d, freq, cum);
      qm_update_store(m, N, sym, slot, fresh);
      const u8 q = (u8)(da.rev[sym] + 33);
#if FQ_WAVE > 1
      if (FQ_LANE == (u32)(op & 63)) obyte = q;
      ++op;
      if ((op & 63) == 0) qd_flush(da.out, op - 64, o_lo, o_hi, obyte);
#else
      da.out[op++] = q;
#endif
      hist = ((hist << cfg.bits) + sym) & cfg.ctx_mask;   // update_context, quality.cpp:209-215
      if (i + 1 < size) slot = qd_open(cfg, tab, ((i + 1) << 48) + hist, sym, ah, la, m, fresh);
    }
    FQ_SYNC_MEM();   // the models written in this read are read again in the next ones
  }
#if FQ_WAVE > 1
  if ((op & 63) != 0) qd_flush(da.out, op & ~63ull, o_lo, op, obyte);   // (the lanes at and beyond op are outside [o_lo, op))
#endif
  if (FQ_LANE == 0) {
    cfg.filled[tid] = filled;
    if (err) *cfg.err = err;
  }
}
