// rc_driver.hip -- test-only entry points into fqsx_rc.h (tests/test_rc_device.py): the exact u64 / u16 division, one
// rc_step from a set state, whole encoder streams (with undersized buffers) and the decoder.  Compiled by the test itself,
// for gfx950 with hipcc and -- FQSX_EMU -- for the host with g++, and loaded with ctypes; no part of the product library.
// The kernels only call what fqsx_rc.h defines; everything a test compares against is computed in Python.
#include "../../fqsqueezer_amd/csrc/fqsx_rc.h"
#include "../../fqsqueezer_amd/csrc/fqsx_rt.h"

// ---- a. division: item i = (divisor d_lo + i / nx, operand i % nx of that divisor) ------------------------------------------
// the first nc operands are the same for every divisor (xc), the other np its own (xp[(d - d_lo) * np ...])
FQ_KERNEL256 void k_rcdrv_div(const u64 *xc, u32 nc, const u64 *xp, u32 np, u32 d_lo, u64 n_items, u64 *q, u64 *recip) {
  const u64 nx = (u64)nc + np, stride = FQ_GRID_STRIDE(u64);
  for (u64 i = FQ_GRID_FIRST(u64); i < n_items; i += stride) {
    const u64 di = i / nx;
    const u32 j = (u32)(i - di * nx), d = d_lo + (u32)di;
    const u64 x = j < nc ? xc[j] : xp[di * np + (j - nc)];
    q[i] = div_u64_small(x, d);
    if (j == 0) recip[di] = d >= 2 ? recip64_u16(d) : 0;
  }
}

// ---- b. one rc_step from a set state, every lane of the wave with the same arguments ------------------------------------------
// result of case c: res[3c ..] = low, range, len; its bytes in out[16c .. 16c + 16)
FQ_KERNEL64 void k_rcdrv_step(u64 n, const u64 *low, const u64 *range, const u32 *freq, const u32 *cum, const u32 *tot, u64 *res, u8 *out) {
  for (u64 c = FQ_BLOCK; c < n; c += FQ_NBLOCKS) {
    RcEnc e;
    rc_open(e, out + 16 * c, 16);
    e.low = low[c];
    e.range = range[c];
    rc_step(e, freq[c], cum[c], tot[c], recip64_u16(tot[c]));
    rc_close(e);
    if (FQ_LANE == 0) { res[3 * c] = e.low; res[3 * c + 1] = e.range; res[3 * c + 2] = e.len; }
  }
}

// ---- c. encoder streams: workgroup s codes script s into buf + out_off[s] (capacity cap[s]) ----------------------------------
FQ_KERNEL64 void k_rcdrv_encode(const u64 *script_off, const u32 *freq, const u32 *cum, const u32 *tot, u8 *buf, const u64 *out_off, const u64 *cap,
                                u64 *len_out, u32 *ovf_out) {
  const u32 s = FQ_BLOCK;
  RcEnc e;
  rc_open(e, buf + out_off[s], cap[s]);
  for (u64 i = script_off[s]; i < script_off[s + 1]; ++i) rc_step(e, freq[i], cum[i], tot[i], recip64_u16(tot[i]));
  rc_end(e);
  if (FQ_LANE == 0) { len_out[s] = e.len; ovf_out[s] = rc_overflowed(e) ? 1u : 0u; }
}

// ---- d. decoder over a plain byte source (bytes past the end of the stream read as 0) ----------------------------------------
struct ByteSrc { const u8 *p; u64 pos, len; };
FQ_DEV u64 rc_src_byte(ByteSrc &s) {
  const u64 b = s.pos < s.len ? s.p[s.pos] : 0;
  ++s.pos;
  return b;
}
// workgroup s decodes script s from its stream; got[i] = what rcd_cum returned at step i, the update is made with the script's
// (freq, cum) -- which symbol a value stands for is the caller's business in the product as well
FQ_KERNEL64 void k_rcdrv_decode(const u64 *script_off, const u32 *freq, const u32 *cum, const u32 *tot, const u8 *streams, const u64 *st_off,
                                const u64 *st_len, u32 *got) {
  const u32 s = FQ_BLOCK;
  ByteSrc src = {streams + st_off[s], 0, st_len[s]};
  RcDec d;
  rcd_start(d, src, st_len[s]);
  for (u64 i = script_off[s]; i < script_off[s + 1]; ++i) {
    const u32 v = rcd_cum(d, tot[i]);
    if (FQ_LANE == 0) got[i] = v;
    rcd_update(d, src, freq[i], cum[i]);
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
namespace {
struct Ctx {
  DevCtx c;
  int rc;
  Ctx() { rc = dev_open(&c, 0); }
  ~Ctx() { if (!rc) dev_close(&c); }
};
// a device copy of n elements of host array h (n == 0: a valid, unused allocation)
template <class E> int upload(DevCtx *c, E *&d, const E *h, u64 n) {
  void *p = nullptr;
  DEVCHK(dalloc(c, &p, n * sizeof(E), false));
  d = (E *)p;
  return n ? h2d(c, p, h, n * sizeof(E)) : FQSX_OK;
}
template <class E> int scratch(DevCtx *c, E *&d, u64 n, bool zero = true) {
  void *p = nullptr;
  DEVCHK(dalloc(c, &p, n * sizeof(E), zero));
  d = (E *)p;
  return FQSX_OK;
}
int fail(const char *what) { g_err = what; return FQSX_E_ARG; }

// Does the renormalisation of this coding step end, with at most 16 bytes written?  The coder's own loop has no bound (a range
// of 0 never grows), so a case is looked at with plain u64 arithmetic on the host before it goes anywhere near a GPU.
// dq: the same question for a quotient that is off by that much.
bool step_ends(u64 &low, u64 &range, u32 freq, u32 cum, u32 tot, int dq = 0) {   // (low, range: the state, advanced by the step)
  const u64 Top = 0x00ffffffffffffULL, M = 0xff00000000000000ULL;
  range = range / tot + (u64)(int64_t)dq;
  low += range * cum;
  range *= freq;
  for (u32 n = 0; range <= Top; ++n) {
    if (n == 16) return false;
    if ((low ^ (low + range)) & M) range = (low | Top) - low;
    low <<= 8;
    range <<= 8;
  }
  return true;
}
bool script_ok(const u64 *script_off, u32 n_scripts, const u32 *freq, const u32 *cum, const u32 *tot) {
  for (u32 s = 0; s < n_scripts; ++s)
    if (script_off[s] > script_off[s + 1]) return false;
  if (script_off[0] != 0) return false;
  for (u32 s = 0; s < n_scripts; ++s) {   // (low and range of the encoder and of the decoder go the same way)
    u64 low = 0, range = 0xff00000000000000ULL;
    for (u64 i = script_off[s]; i < script_off[s + 1]; ++i) {
      if (tot[i] < 2 || tot[i] > 0xffff || freq[i] == 0 || (u64)cum[i] + freq[i] > tot[i]) return false;
      if (!step_ends(low, range, freq[i], cum[i], tot[i])) return false;
    }
  }
  return true;
}

int run_div(DevCtx *c, const u64 *xc, u32 nc, const u64 *xp, u32 np, u32 d_lo, u32 d_hi, u64 *q, u64 *recip) {
  if (d_lo < 1 || d_hi < d_lo || d_hi > 0xffff || nc + np == 0) return fail("rcdrv_div: divisors 1 .. 65535, at least one operand");
  const u64 nd = (u64)d_hi - d_lo + 1, n_items = nd * ((u64)nc + np);
  u64 *d_xc, *d_xp, *d_q, *d_r;
  DEVCHK(upload(c, d_xc, xc, (u64)nc));
  DEVCHK(upload(c, d_xp, xp, nd * np));
  DEVCHK(scratch(c, d_q, n_items, false));
  DEVCHK(scratch(c, d_r, nd, false));
  const u32 grid = (u32)std::min<u64>((n_items + 255) / 256, 1u << 16);
  LAUNCH(c, 0, k_rcdrv_div, FQ_GRID(grid), 256, d_xc, nc, d_xp, np, d_lo, n_items, d_q, d_r);
  DEVCHK(d2h(c, q, d_q, n_items * 8));
  return d2h_sync(c, recip, d_r, nd * 8);
}

int run_step(DevCtx *c, u64 n, const u64 *low, const u64 *range, const u32 *freq, const u32 *cum, const u32 *tot, u64 *res, u8 *out) {
  if (n == 0) return fail("rcdrv_step: no cases");
  for (u64 i = 0; i < n; ++i) {
    if (tot[i] < 2 || tot[i] > 0xffff || freq[i] == 0 || (u64)cum[i] + freq[i] > tot[i]) return fail("rcdrv_step: not a (freq, cum, tot) of a model");
    if (range[i] <= 0x00ffffffffffffULL) return fail("rcdrv_step: a range below 2^48 is no state of the coder");
    // (also with a quotient one off: a defect in the coder's division should come back as wrong numbers, not hang a wave)
    for (int dq = -1; dq <= 1; ++dq) {
      u64 l = low[i], r = range[i];
      if (!step_ends(l, r, freq[i], cum[i], tot[i], dq)) return fail("rcdrv_step: the renormalisation of a case does not end");
    }
  }
  u64 *d_low, *d_range, *d_res;
  u32 *d_freq, *d_cum, *d_tot;
  u8 *d_out;
  DEVCHK(upload(c, d_low, low, n));
  DEVCHK(upload(c, d_range, range, n));
  DEVCHK(upload(c, d_freq, freq, n));
  DEVCHK(upload(c, d_cum, cum, n));
  DEVCHK(upload(c, d_tot, tot, n));
  DEVCHK(scratch(c, d_res, 3 * n));
  DEVCHK(scratch(c, d_out, 16 * n));
  LAUNCH(c, 0, k_rcdrv_step, (u32)std::min<u64>(n, 1u << 15), 64, n, d_low, d_range, d_freq, d_cum, d_tot, d_res, d_out);
  DEVCHK(d2h(c, res, d_res, 3 * n * 8));
  return d2h_sync(c, out, d_out, 16 * n);
}

int run_encode(DevCtx *c, u32 n_scripts, const u64 *script_off, const u32 *freq, const u32 *cum, const u32 *tot, u8 *buf, u64 buf_bytes,
               const u64 *out_off, const u64 *cap, u64 *len_out, u32 *ovf_out) {
  if (n_scripts == 0 || !script_ok(script_off, n_scripts, freq, cum, tot)) return fail("rcdrv_encode: bad scripts");
  for (u32 s = 0; s < n_scripts; ++s)   // the coder stores aligned 8-byte words below cap: all of them inside the caller's buffer
    if ((out_off[s] & 7) || (cap[s] & 7) || out_off[s] > buf_bytes || cap[s] > buf_bytes - out_off[s]) return fail("rcdrv_encode: stream outside the buffer or unaligned");
  const u64 n_sym = script_off[n_scripts];
  u64 *d_soff, *d_ooff, *d_cap, *d_len;
  u32 *d_freq, *d_cum, *d_tot, *d_ovf;
  u8 *d_buf;
  DEVCHK(upload(c, d_soff, script_off, (u64)n_scripts + 1));
  DEVCHK(upload(c, d_freq, freq, n_sym));
  DEVCHK(upload(c, d_cum, cum, n_sym));
  DEVCHK(upload(c, d_tot, tot, n_sym));
  DEVCHK(upload(c, d_buf, (const u8 *)buf, buf_bytes));
  DEVCHK(upload(c, d_ooff, out_off, (u64)n_scripts));
  DEVCHK(upload(c, d_cap, cap, (u64)n_scripts));
  DEVCHK(scratch(c, d_len, (u64)n_scripts));
  DEVCHK(scratch(c, d_ovf, (u64)n_scripts));
  LAUNCH(c, 0, k_rcdrv_encode, n_scripts, 64, d_soff, d_freq, d_cum, d_tot, d_buf, d_ooff, d_cap, d_len, d_ovf);
  if (buf_bytes) DEVCHK(d2h(c, buf, d_buf, buf_bytes));
  DEVCHK(d2h(c, len_out, d_len, (u64)n_scripts * 8));
  return d2h_sync(c, ovf_out, d_ovf, (u64)n_scripts * 4);
}

int run_decode(DevCtx *c, u32 n_scripts, const u64 *script_off, const u32 *freq, const u32 *cum, const u32 *tot, const u8 *streams,
               u64 stream_bytes, const u64 *st_off, const u64 *st_len, u32 *got) {
  if (n_scripts == 0 || !script_ok(script_off, n_scripts, freq, cum, tot)) return fail("rcdrv_decode: bad scripts");
  for (u32 s = 0; s < n_scripts; ++s)
    if (st_len[s] < 8 || st_off[s] > stream_bytes || st_len[s] > stream_bytes - st_off[s]) return fail("rcdrv_decode: stream outside the buffer or shorter than 8 bytes");
  const u64 n_sym = script_off[n_scripts];
  u64 *d_soff, *d_stoff, *d_stlen;
  u32 *d_freq, *d_cum, *d_tot, *d_got;
  u8 *d_st;
  DEVCHK(upload(c, d_soff, script_off, (u64)n_scripts + 1));
  DEVCHK(upload(c, d_freq, freq, n_sym));
  DEVCHK(upload(c, d_cum, cum, n_sym));
  DEVCHK(upload(c, d_tot, tot, n_sym));
  DEVCHK(upload(c, d_st, streams, stream_bytes));
  DEVCHK(upload(c, d_stoff, st_off, (u64)n_scripts));
  DEVCHK(upload(c, d_stlen, st_len, (u64)n_scripts));
  DEVCHK(scratch(c, d_got, n_sym));
  LAUNCH(c, 0, k_rcdrv_decode, n_scripts, 64, d_soff, d_freq, d_cum, d_tot, d_st, d_stoff, d_stlen, d_got);
  return d2h_sync(c, got, d_got, n_sym * 4);
}
}  // namespace

extern "C" {
const char *rcdrv_error() { return g_err.c_str(); }
// 1: compiled for the GPU (hardware reciprocal, 64 lanes), 0: the emulation
int rcdrv_is_gpu() {
#ifndef FQSX_EMU
  return 1;
#else
  return 0;
#endif
}
// q[(d - d_lo) * (nc + np) + j] = div_u64_small(x_j of d, d), recip[d - d_lo] = recip64_u16(d) (0 for d = 1)
int rcdrv_div(const u64 *xc, u32 nc, const u64 *xp, u32 np, u32 d_lo, u32 d_hi, u64 *q, u64 *recip) {
  Ctx x;
  return x.rc ? x.rc : run_div(&x.c, xc, nc, xp, np, d_lo, d_hi, q, recip);
}
// case i: res[3i ..] = low, range, len after one rc_step from (low[i], range[i]); out[16i ..]: the bytes it wrote
int rcdrv_step(u64 n, const u64 *low, const u64 *range, const u32 *freq, const u32 *cum, const u32 *tot, u64 *res, u8 *out) {
  Ctx x;
  return x.rc ? x.rc : run_step(&x.c, n, low, range, freq, cum, tot, res, out);
}
// script s = symbols script_off[s] .. script_off[s + 1]; its stream goes to buf + out_off[s], capacity cap[s] (both multiples of 8)
int rcdrv_encode(u32 n_scripts, const u64 *script_off, const u32 *freq, const u32 *cum, const u32 *tot, u8 *buf, u64 buf_bytes,
                 const u64 *out_off, const u64 *cap, u64 *len_out, u32 *ovf_out) {
  Ctx x;
  return x.rc ? x.rc : run_encode(&x.c, n_scripts, script_off, freq, cum, tot, buf, buf_bytes, out_off, cap, len_out, ovf_out);
}
// got[i] = rcd_cum at symbol i of the scripts, decoding script s from streams[st_off[s] .. + st_len[s])
int rcdrv_decode(u32 n_scripts, const u64 *script_off, const u32 *freq, const u32 *cum, const u32 *tot, const u8 *streams, u64 stream_bytes,
                 const u64 *st_off, const u64 *st_len, u32 *got) {
  Ctx x;
  return x.rc ? x.rc : run_decode(&x.c, n_scripts, script_off, freq, cum, tot, streams, stream_bytes, st_off, st_len, got);
}
}
