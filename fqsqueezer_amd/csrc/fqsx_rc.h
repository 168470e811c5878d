// fqsx_rc.h -- the range coder on the device, once (CRangeEncoder / CRangeDecoder, sub_rc.h:34-158): used by the DNA
// kernels (fqsx_dev.h, fqsx_dec.h) and by the quality and id kernels (fqsx_qual.h, fqsx_qdec.h, fqsx_idk.h, fqsx_iddec.h).
// The coder state is wave-uniform.  Everything here is force-inlined and takes its state by reference, so that a caller
// that keeps the state in scalar registers (the DNA encoder, see enc_open) keeps it there.  The host twins the kernels are
// tested against (fqsx_host.cpp, oracle/) deliberately share nothing with this file.
#pragma once
#include "fqsx_plat.h"

// ---- exact u64 / u16 ----------------------------------------------------------------------------------------------------
// exact x / d for d < 2^16 without the 64-bit software divide or an IEEE fp64 division: hardware
// reciprocal (~26 bits) + one Newton step (~52 bits), high word and the remaining < 2^48 dividend each by one fp64
// multiply with a +-1 fix-up (sub_rc.h:63).  tools/ubench checks it against u64 division on 1.3e9 operands.
FQ_DEV double recip_u16(u32 d) {
  const double dd = (double)d;
#ifndef FQSX_EMU
  const double r0 = __builtin_amdgcn_rcp(dd);
  return __builtin_fma(r0, __builtin_fma(-dd, r0, 1.0), r0);
#else
  return 1.0 / dd;
#endif
}
FQ_DEV u64 div_u64_rd(u64 x, u32 d, double rd) {
  const u32 hi = (u32)(x >> 32), lo = (u32)x;
  u32 qh = (u32)((double)hi * rd);
  u32 ph = qh * d;
  if (ph > hi) { --qh; ph -= d; } else if (hi - ph >= d) { ++qh; ph += d; }
  const u32 r1 = hi - ph;                                                        // < d
  const double remd = __builtin_fma((double)r1, 4294967296.0, (double)lo);      // exact: < 2^48
  u32 q = (u32)(remd * rd);                                                      // rem / d < 2^32
  const u64 rem = ((u64)r1 << 32) | lo;
  const u64 prod = (u64)q * d;
  if (prod > rem) --q;
  else if (rem - prod >= d) ++q;
  return ((u64)qh << 32) + q;
}
FQ_DEV u64 div_u64_small(u64 x, u32 d) { return div_u64_rd(x, d, recip_u16(d)); }
// m = floor((2^64-1) / tot) of a coding step (rc_step), computed off the coder's chain where the caller can
FQ_DEV u64 recip64_u16(u32 d) { return div_u64_rd(~0ull, d, recip_u16(d)); }

// ---- encoder ------------------------------------------------------------------------------------------------------------
// Output bytes are gathered into the aligned 8-byte word they belong to (acc) and leave with one store per word; the
// stream starts at offset 0 of an aligned buffer of `cap` bytes.  Words that do not fit are dropped while len goes on
// counting: the stream has overflowed exactly when len > cap (there is no error flag beside it).
struct RcEnc { u64 low, range, len, cap, acc; u8 *out; };
FQ_DEV void rc_open(RcEnc &e, u8 *out, u64 cap) {   // a new stream (application.cpp:624-628)
  e.low = 0; e.range = 0xff00000000000000ULL; e.len = 0; e.acc = 0; e.cap = cap; e.out = out;
}
FQ_DEV bool rc_overflowed(const RcEnc &e) { return e.len > e.cap; }
FQ_DEV void rc_byte(RcEnc &e, u8 b) {
  e.acc |= (u64)b << (8 * (u32)(e.len & 7));
  ++e.len;
  if ((e.len & 7) == 0) {
    if (e.len <= e.cap) ((u64 *)e.out)[(e.len >> 3) - 1] = e.acc;
    e.acc = 0;
  }
}
FQ_DEV void rc_close(RcEnc &e) {   // the partly filled word (its tail is rewritten when the stream goes on)
  if ((e.len & 7) && e.len < e.cap) ((u64 *)e.out)[e.len >> 3] = e.acc;
}
FQ_DEV void rc_end(RcEnc &e) {   // End(), sub_rc.h:79-86
  for (int i = 0; i < 8; ++i) { rc_byte(e, (u8)(e.low >> 56)); e.low <<= 8; }
  rc_close(e);
}
// One coding step (Encode, sub_rc.h:60-77) with the division as an integer multiply-high by
// m = floor((2^64-1) / tot), 2 <= tot < 2^16: for any range < 2^64, mulhi(range, m) is the quotient or one less.
// Integer only: with wave-uniform arguments the whole dependent chain of a symbol runs on the scalar unit.
FQ_DEV void rc_step(RcEnc &e, u32 freq, u32 cum, u32 tot, u64 m) {
  const u64 Top = 0x00ffffffffffffULL, M = 0xff00000000000000ULL;
  u64 low = e.low;
#ifndef FQSX_EMU
  u64 range = __umul64hi(e.range, m);
#else
  u64 range = (u64)(((unsigned __int128)e.range * m) >> 64);
#endif
  // mulhi gives the quotient or one less, so the remainder is below 2 * tot < 2^17: its low 32 bits decide (one
  // multiply, one subtract, one compare on the scalar unit instead of a 64-bit multiply-subtract-compare)
  if ((u32)e.range - (u32)range * tot >= tot) ++range;
  low += range * cum;
  range *= freq;
  while (range <= Top) {
    if ((low ^ (low + range)) & M) range = (low | Top) - low;
    rc_byte(e, (u8)(low >> 56));
    low <<= 8;
    range <<= 8;
  }
  e.low = low;
  e.range = range;
}

// ---- decoder ------------------------------------------------------------------------------------------------------------
// The arithmetic of CRangeDecoder; the bytes come from the caller's rc_src_byte(src) (bytes beyond the stream read as 0): the DNA
// decoder reads single bytes (Wk, fqsx_dec.h), the quality and id decoders aligned words one word ahead (QDec, fqsx_qdec.h).
struct RcDec { u64 low, range, buf; };
template <class Src>
FQ_DEV void rcd_start(RcDec &d, Src &src, u64 len) {  // Start(), sub_rc.h:112-125
  d.buf = 0;
  if (len >= 8)
    for (u32 i = 1; i <= 8; ++i) d.buf |= rc_src_byte(src) << (64 - i * 8);
  d.low = 0;
  d.range = 0xff00000000000000ULL;
}
// GetCumulativeFreq, sub_rc.h:127-131.  A well-formed stream gives a value below tot; a quotient beyond 32 bits (malformed
// stream) is clamped, which the callers treat like any other value >= tot.
FQ_DEV u32 rcd_cum(RcDec &d, u32 tot) {
  d.range = div_u64_small(d.range, tot);
  const u64 q = d.buf / d.range;   // (range > 2^56 before the division and tot < 2^16: never 0)
  return q > 0xffffffffull ? 0xffffffffu : (u32)q;
}
template <class Src>
FQ_DEV void rcd_update(RcDec &d, Src &src, u32 freq, u32 cum) {  // UpdateFrequency, sub_rc.h:133-151
  const u64 Top = 0x00ffffffffffffULL, M = 0xff00000000000000ULL;
  const u64 r = (u64)cum * d.range;
  u64 low = d.low + r, range = d.range * freq;
  d.buf -= r;
  while (range <= Top) {
    if ((low ^ (low + range)) & M) range = (low | Top) - low;
    d.buf = (d.buf << 8) + rc_src_byte(src);
    low <<= 8;
    range <<= 8;
  }
  d.low = low;
  d.range = range;
}
