// fqsx_fqtext.h -- columns to FASTQ text on the GPU: the last step of reading a .fqs file back, the inverse of fqsx_fastq.h.
//
// The reference writes a decoded read as id line (with its line feed) + bases + "\n+\n" + qualities + "\n", and the reads
// of a paired block alternately to its two outputs (application.cpp:871-889, 980-982).  Same text here, from the columns
// the decoders leave in device memory (the id lines back to back with their lengths, the bases and the qualities back to
// back under one offset array), as scan-and-scatter passes over the records of a container block:
//   k_ft_sizes        per record its checks (offsets ascending, a read below 2^24 bases, an id line of at least its line
//                     feed) and its size id_len + 2 L + 4; per tile of 2048 records the sum of the sizes per output, of the
//                     id lengths and of the read lengths
//   k_ft_scan_tiles   exclusive scan of those tile sums (one workgroup), the block's totals
//   k_ft_offsets      per record its start in its output and the start of its id line
//   k_ft_scatter      the lanes of a wave look up one record each and check its ranges; then the wave copies its records,
//                     sixteen lanes to a record, every piece with cols_copy (16-byte stores from the destination's first
//                     boundary on); the five constant bytes are one lane's
// A record whose range would leave a buffer sets the error word and is not copied, so nothing outside the output buffers
// is ever written.  All sums are 64-bit: a tile of 2048 records of 2^24 bases passes 32 bits, which is why the scans here
// are ft_wg_scan64 and not fq_wg_scan (same shape, wider value).  Workgroups are 256 threads (4 waves); the emulation build
// runs them as one 1-lane wave.
#pragma once
#include "fqsx_fastq.h"
#include "fqsx_cols.h"

#define FQSX_FT_RTILE FQSX_FQ_RTILE   // records per workgroup (sizes / offsets)
#define FQSX_FT_MAX_READ (1u << 24)   // a read of this many bases or more is refused (as the quality decoder refuses it)
// result words of a call: the block's totals and its error flags
enum { FT_RES_TEXT0 = 0, FT_RES_TEXT1 = 1, FT_RES_ID_BYTES = 2, FT_RES_BASES = 3, FT_ERR_OFFSETS = 4, FT_ERR_LENGTH = 5, FT_ERR_ID = 6, FT_ERR_RANGE = 7, FT_N_RES = 8 };
enum { FT_SUM_TEXT0 = 0, FT_SUM_TEXT1 = 1, FT_SUM_ID = 2, FT_SUM_BASES = 3, FT_N_SUM = 4 };

struct FtCfg {
  u32 n, paired;        // records of the block; 1: record i goes to output i & 1
  u32 n_tiles;
  const u8 *ids;        // the id lines back to back, or null: every id line is "@\n"
  const u32 *id_len;    // [n] (unused without ids)
  u64 id_bytes;
  const u8 *bases;      // [n_bases]
  const u8 *quals;      // [n_bases], or null: every quality is the byte `fill`
  u32 fill;
  u64 n_bases;
  const u64 *read_off;  // [n + 1]
  u64 *tile;            // [FT_N_SUM][n_tiles]
  u64 *tile_pre;        // [FT_N_SUM][n_tiles + 1]
  u64 *start;           // [n]: where the record begins in its output
  u64 *id_off;          // [n]: where its id line begins in ids
  u8 *out[2];
  u64 out_n[2];
  u64 *res;             // [FT_N_RES]
};

// Exclusive prefix over the threads of the workgroup of a 64-bit value: fq_wg_scan with wider words.  ws: LDS [FQ_WAVES256].
FQ_DEV u64 ft_wg_scan64(u64 v, u64 *ws, u64 &total) {
  const u64 wave_ex = wave_excl_scan64(v), wave_tot = wave_sum64(v);
  FQ_WG_BARRIER();   // (the call before may still be reading ws)
  if (FQ_LANE == 0) ws[FQ_WAVE_ID] = wave_tot;
  FQ_WG_BARRIER();
  u64 pre = 0, tot = 0;
  for (u32 w = 0; w < FQ_WAVES256; ++w) {
    const u64 x = ws[w];
    pre += w < FQ_WAVE_ID ? x : 0ull;
    tot += x;
  }
  total = tot;
  return pre + wave_ex;
}

// id line and read length of record r (r < n); false, with its error word set, for a record the block is refused for
FQ_DEV bool ft_record(const FtCfg &c, u64 r, u32 &il, u32 &L) {
  const u64 o0 = c.read_off[r], o1 = c.read_off[r + 1];
  il = c.ids ? c.id_len[r] : 2u;
  L = 0;
  if (o1 < o0) { c.res[FT_ERR_OFFSETS] = 1; return false; }
  if (o1 - o0 >= FQSX_FT_MAX_READ) { c.res[FT_ERR_LENGTH] = 1; return false; }
  if (il == 0) { c.res[FT_ERR_ID] = 1; return false; }
  L = (u32)(o1 - o0);
  return true;
}

FQ_KERNEL256 void k_ft_sizes(FtCfg c) {
  FQ_SHARED u64 red[FQ_WAVES256 * FT_N_SUM];
  const u64 lo = (u64)FQ_BLOCK * FQSX_FT_RTILE;
  u64 s[FT_N_SUM] = {0, 0, 0, 0};
  for (u32 j = FQ_T256; j < FQSX_FT_RTILE && lo + j < c.n; j += FQ_N256) {
    const u64 r = lo + j;
    u32 il, L;
    if (!ft_record(c, r, il, L)) continue;
    s[c.paired ? (u32)(r & 1) : 0u] += (u64)il + 2ull * L + 4;
    s[FT_SUM_ID] += il;
    s[FT_SUM_BASES] += L;
  }
  for (u32 k = 0; k < FT_N_SUM; ++k) s[k] = wave_sum64(s[k]);
  if (FQ_LANE == 0)
    for (u32 k = 0; k < FT_N_SUM; ++k) red[FQ_WAVE_ID * FT_N_SUM + k] = s[k];
  FQ_WG_BARRIER();
  for (u32 k = FQ_T256; k < FT_N_SUM; k += FQ_N256) {
    u64 t = 0;
    for (u32 w = 0; w < FQ_WAVES256; ++w) t += red[w * FT_N_SUM + k];
    c.tile[(u64)k * c.n_tiles + FQ_BLOCK] = t;
  }
}

// one workgroup, a round of one tile per thread at a time
FQ_KERNEL256 void k_ft_scan_tiles(FtCfg c) {
  FQ_SHARED u64 ws[FQ_WAVES256];
  for (u32 q = 0; q < FT_N_SUM; ++q) {
    u64 run = 0;
    for (u32 b = 0; b < c.n_tiles; b += FQ_N256) {
      const u32 i = b + FQ_T256;
      const u64 v = i < c.n_tiles ? c.tile[(u64)q * c.n_tiles + i] : 0ull;
      u64 tot;
      const u64 ex = ft_wg_scan64(v, ws, tot);
      if (i < c.n_tiles) c.tile_pre[(u64)q * (c.n_tiles + 1) + i] = run + ex;
      run += tot;
    }
    if (FQ_T256 == 0) {
      c.tile_pre[(u64)q * (c.n_tiles + 1) + c.n_tiles] = run;
      c.res[FT_RES_TEXT0 + q] = run;
    }
  }
}

FQ_KERNEL256 void k_ft_offsets(FtCfg c) {
  FQ_SHARED u64 ws[FQ_WAVES256];
  const u64 lo = (u64)FQ_BLOCK * FQSX_FT_RTILE;
  u64 run[3];
  for (u32 q = 0; q < 3; ++q) run[q] = c.tile_pre[(u64)q * (c.n_tiles + 1) + FQ_BLOCK];
  for (u32 j0 = 0; j0 < FQSX_FT_RTILE && lo + j0 < c.n; j0 += FQ_N256) {
    const u64 r = lo + j0 + FQ_T256;
    u32 il = 0, L = 0;
    const bool ok = r < c.n && ft_record(c, r, il, L);
    const u64 size = ok ? (u64)il + 2ull * L + 4 : 0ull;
    const u32 m = c.paired ? (u32)(r & 1) : 0u;
    u64 tot, mine = 0;
    for (u32 q = 0; q < (c.paired ? 2u : 1u); ++q) {
      const u64 ex = ft_wg_scan64(q == m ? size : 0ull, ws, tot);
      if (q == m) mine = run[q] + ex;
      run[q] += tot;
    }
    if (r < c.n) c.start[r] = mine;
    if (c.ids) {
      const u64 ex = ft_wg_scan64(ok ? il : 0u, ws, tot);
      if (r < c.n) c.id_off[r] = run[2] + ex;
      run[2] += tot;
    }
  }
}

struct FtRec { u64 dst, ids, seq; u32 il, L, ok; };   // start in out[m] | m << 63, start of the id line, of the bases; ok = 0: not copied

// record i of the block: where its pieces come from and where they go, ok = 0 unless every range lies inside its buffer
FQ_DEV FtRec ft_lookup(const FtCfg &c, u64 i) {
  FtRec r = {0, 0, 0, 0, 0, 0};
  if (i >= c.n) return r;
  if (!ft_record(c, i, r.il, r.L)) return r;
  const u32 m = c.paired ? (u32)(i & 1) : 0u;
  const u64 size = (u64)r.il + 2ull * r.L + 4, d = c.start[i], so = c.read_off[i];
  if (d > c.out_n[m] || size > c.out_n[m] - d) { c.res[FT_ERR_RANGE] = 1; return r; }
  if (so > c.n_bases || r.L > c.n_bases - so) { c.res[FT_ERR_RANGE] = 1; return r; }
  if (c.ids) {
    r.ids = c.id_off[i];
    if (r.ids > c.id_bytes || r.il > c.id_bytes - r.ids) { c.res[FT_ERR_RANGE] = 1; return r; }
  }
  r.dst = d | ((u64)m << 63);
  r.seq = so;
  r.ok = 1;
  return r;
}

// len bytes `byte` at dst by the COLS_SUB lanes of a record: cols_copy's split without a source
FQ_DEV void ft_fill(u8 *dst, u32 byte, u32 len, u32 sl) {
  const u32 to_boundary = (u32)((16u - ((u64)(uintptr_t)dst & 15u)) & 15u), head = to_boundary < len ? to_boundary : len;
  const u32 groups = (len - head) / 16u, tail = head + 16u * groups;
  const u64 w = 0x0101010101010101ull * (byte & 0xffu);
  const Cols16 v = {w, w};
  for (u32 p = sl; p < head; p += COLS_SUB) dst[p] = (u8)byte;
  for (u32 g = sl; g < groups; g += COLS_SUB) *(Cols16 *)(dst + head + 16u * g) = v;
  for (u32 p = tail + sl; p < len; p += COLS_SUB) dst[p] = (u8)byte;
}

FQ_KERNEL256 void k_ft_scatter(FtCfg c) {
  const u64 i0 = ((u64)FQ_BLOCK * COLS_WAVES + FQ_WAVE_ID) * FQ_WAVE;
  const FtRec mine = ft_lookup(c, i0 + FQ_LANE);
  for (u32 j0 = 0; j0 < FQ_WAVE; j0 += FQ_WAVE / COLS_SUB) {
    const u32 from = j0 + FQ_LANE / COLS_SUB, sl = FQ_LANE % COLS_SUB;
    const u32 ok = wave_bcast32(mine.ok, from), il = wave_bcast32(mine.il, from), L = wave_bcast32(mine.L, from);
    const u64 d = wave_bcast64(mine.dst, from), io = wave_bcast64(mine.ids, from), so = wave_bcast64(mine.seq, from);
    if (!ok) continue;
    u8 *dst = c.out[d >> 63] + (d & ~(1ull << 63));
    if (c.ids) cols_copy(dst, c.ids + io, il, sl);
    else if (sl == 0) { dst[0] = '@'; dst[1] = '\n'; }
    cols_copy(dst + il, c.bases + so, L, sl);
    u8 *q = dst + il + L + 3;
    if (c.quals) cols_copy(q, c.quals + so, L, sl);
    else ft_fill(q, c.fill, L, sl);
    if (sl == 0) { q[-3] = '\n'; q[-2] = '+'; q[-1] = '\n'; q[L] = '\n'; }
  }
}
