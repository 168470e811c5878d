// fqsx_fastq.h -- FASTQ text to columns on the GPU: the ingestion step in front of the coders.
//
// The reference reads a record byte by byte (CReadsBlock::get_read, reads_block.h:35-76; CSortedFASTQFile::get_read,
// io.h:451-482): a line ends at 0x0A and nowhere else (a 0x0D stays in its field), four line feeds make a record, and
// what follows the last fourth line feed is no record.  Same rule here, as scan-and-gather passes over a chunk of text
// in device memory:
//   k_fq_count        line feeds per 16 KiB tile of text (16-byte loads)
//   k_fq_scan_tiles   exclusive scan of the tile counts (one workgroup, 64-bit totals)
//   k_fq_index        line_end[rank] = byte position of the rank-th line feed (ballot + popcount of the lower lanes)
//   k_fq_lengths      per record the four field lengths; per tile of records their sums, the longest id line and
//                     whether a quality line differs in length from its base line
//   k_fq_scan_rtiles  scan of those tile sums, the chunk's summary (records, bytes consumed, column sizes)
//   k_fq_offsets      id_off / read_off / qual_off: exclusive scans of the id, base and quality lengths
//   k_fq_gather       every field copied into its column, the lanes of a wave across the bytes of a record
// Workgroups are 256 threads (4 waves); the emulation build runs them as one 1-lane wave, so everything that crosses
// lanes or waves goes through the wave primitives of fqsx_plat.h and fq_wg_scan below.
#pragma once
#include "fqsx_plat.h"

#define FQSX_FQ_TILE 16384u     // bytes of text per workgroup (count / index)
#define FQSX_FQ_RTILE 2048u     // records per workgroup (lengths / offsets)
#define FQSX_FQ_GBATCH 64u      // records per wave (gather): a workgroup takes 4 batches
#ifndef FQSX_EMU
#define FQ_WAVES256 4u
#else
#define FQ_WAVES256 1u
#endif
#define FQ_T256 (FQ_WAVE_ID * FQ_WAVE + FQ_LANE)   // thread of the workgroup
#define FQ_N256 (FQ_WAVES256 * FQ_WAVE)            // threads of the workgroup
enum { FQ_LEN_ID = 0, FQ_LEN_BASES = 1, FQ_LEN_PLUS = 2, FQ_LEN_QUAL = 3 };
enum { FQ_SUM_RECORDS = 0, FQ_SUM_CONSUMED = 1, FQ_SUM_ID_BYTES = 2, FQ_SUM_BASES = 3, FQ_SUM_QUALS = 4, FQ_SUM_MAX_ID = 5, FQ_SUM_MISMATCH = 6, FQ_SUM_LINE_FEEDS = 7 };

struct FqCfg {
  const u8 *text;   // [n], 16-byte aligned
  u64 n;
  u32 n_tiles;
  u32 *tile_cnt;    // [n_tiles]
  u64 *tile_pre;    // [n_tiles + 1]
  u64 *line_end;    // [n_lf]
  u64 n_lf, n_rec;
  u32 *len;         // [4][len_stride]: id line (with its line feed), bases, separator line, qualities
  u64 len_stride;
  u32 n_rtiles;
  u32 *rt;          // [5][n_rtiles]: sums of the id / base / quality lengths, longest id line, length mismatch seen
  u64 *rt_pre;      // [3][n_rtiles + 1]
  u64 *off;         // [3][off_stride]: id_off, read_off, qual_off, n_rec + 1 entries each
  u64 off_stride;
  u8 *col[3];       // ids, bases, quals
  u64 col_n[3];     // ... and their sizes
  u64 *summary;     // [8], FQ_SUM_*
};

struct alignas(16) FqText16 { u64 lo, hi; };

// bit k = byte k of w (little endian: text order) is 0x0A
FQ_DEV u32 fq_lf_bits8(u64 w) {
  const u64 x = w ^ 0x0a0a0a0a0a0a0a0aull, k = 0x7f7f7f7f7f7f7f7full;
  const u64 z = ~(((x & k) + k) | x | k);   // 0x80 in exactly the bytes of x that are zero
  return (u32)(((z >> 7) * 0x0102040810204080ull) >> 56);
}
// bit k = text[pos + k] is a line feed, k < 16; pos is a multiple of 16 and below n; nothing at or past n is read
FQ_DEV u32 fq_lf_mask16(const u8 *text, u64 pos, u64 n) {
  if (pos + 16 <= n) {
    const FqText16 v = *(const FqText16 *)(text + pos);
    return fq_lf_bits8(v.lo) | (fq_lf_bits8(v.hi) << 8);
  }
  u32 m = 0;
  for (u32 k = 0; pos + k < n; ++k) m |= (text[pos + k] == 0x0a ? 1u : 0u) << k;
  return m;
}
// Exclusive prefix over the threads of the workgroup, in thread order, of a value whose prefix inside the wave (wave_ex) and
// whose wave total (wave_tot) the caller has; total: the workgroup's sum.  ws: LDS [FQ_WAVES256].  Every thread calls it.
FQ_DEV u32 fq_wg_scan(u32 wave_ex, u32 wave_tot, u32 *ws, u32 &total) {
  FQ_WG_BARRIER();   // (the call before may still be reading ws)
  if (FQ_LANE == 0) ws[FQ_WAVE_ID] = wave_tot;
  FQ_WG_BARRIER();
  u32 pre = 0, tot = 0;
  for (u32 w = 0; w < FQ_WAVES256; ++w) {
    const u32 x = ws[w];
    pre += w < FQ_WAVE_ID ? x : 0u;
    tot += x;
  }
  total = tot;
  return pre + wave_ex;
}

FQ_KERNEL256 void k_fq_count(FqCfg c) {
  FQ_SHARED u32 ws[FQ_WAVES256];
  const u64 base = (u64)FQ_BLOCK * FQSX_FQ_TILE;
  u32 cnt = 0;
  for (u32 u = FQ_T256; u < FQSX_FQ_TILE / 16; u += FQ_N256) {
    const u64 pos = base + 16ull * u;
    if (pos < c.n) cnt += popc64(fq_lf_mask16(c.text, pos, c.n));
  }
  cnt = wave_sum32(cnt);
  if (FQ_LANE == 0) ws[FQ_WAVE_ID] = cnt;
  FQ_WG_BARRIER();
  if (FQ_T256 == 0) {
    u32 s = 0;
    for (u32 w = 0; w < FQ_WAVES256; ++w) s += ws[w];
    c.tile_cnt[FQ_BLOCK] = s;
  }
}

// one workgroup: 16 GiB of text in 16 KiB tiles is 2^20 counts
FQ_KERNEL256 void k_fq_scan_tiles(FqCfg c) {
  FQ_SHARED u32 ws[FQ_WAVES256];
  u64 run = 0;
  for (u32 b = 0; b < c.n_tiles; b += FQ_N256) {
    const u32 i = b + FQ_T256;
    const u32 v = i < c.n_tiles ? c.tile_cnt[i] : 0u;
    u32 tot;
    const u32 ex = fq_wg_scan(wave_excl_scan32(v), wave_sum32(v), ws, tot);
    if (i < c.n_tiles) c.tile_pre[i] = run + ex;
    run += tot;
  }
  if (FQ_T256 == 0) {
    c.tile_pre[c.n_tiles] = run;
    c.summary[FQ_SUM_LINE_FEEDS] = run;
  }
}

FQ_KERNEL256 void k_fq_index(FqCfg c) {
  FQ_SHARED u32 ws[FQ_WAVES256];
  const u64 base = (u64)FQ_BLOCK * FQSX_FQ_TILE;
  const u64 lower = (1ull << FQ_LANE) - 1ull;
  u64 run = c.tile_pre[FQ_BLOCK];
  for (u32 u0 = 0; u0 < FQSX_FQ_TILE / 16 && base + 16ull * u0 < c.n; u0 += FQ_N256) {
    const u64 pos = base + 16ull * (u0 + FQ_T256);
    u32 m = pos < c.n ? fq_lf_mask16(c.text, pos, c.n) : 0u;
    const u32 cnt = popc64(m);
    u32 ex, wtot;
    if (!wave_any(cnt > 1)) {   // lines of 16 bytes and more: at most one line feed per lane
      const u64 b = wave_ballot(cnt != 0);
      ex = popc64(b & lower);
      wtot = popc64(b);
    } else {
      ex = wave_excl_scan32(cnt);
      wtot = wave_sum32(cnt);
    }
    u32 tot;
    u64 rank = run + fq_wg_scan(ex, wtot, ws, tot);
    for (; m; m &= m - 1, ++rank)
      if (rank < c.n_lf) c.line_end[rank] = pos + ctz64(m);
    run += tot;
  }
}

FQ_KERNEL256 void k_fq_lengths(FqCfg c) {
  FQ_SHARED u32 red[FQ_WAVES256 * 5];
  const u64 lo = (u64)FQ_BLOCK * FQSX_FQ_RTILE;
  u32 s_id = 0, s_b = 0, s_q = 0, mx = 0, bad = 0;
  for (u32 j = FQ_T256; j < FQSX_FQ_RTILE && lo + j < c.n_rec; j += FQ_N256) {
    const u64 r = lo + j;
    const u64 start = r ? c.line_end[4 * r - 1] + 1 : 0;
    const u64 e1 = c.line_end[4 * r], e2 = c.line_end[4 * r + 1], e3 = c.line_end[4 * r + 2], e4 = c.line_end[4 * r + 3];
    const u32 l_id = (u32)(e1 - start + 1), l_b = (u32)(e2 - e1 - 1), l_p = (u32)(e3 - e2 - 1), l_q = (u32)(e4 - e3 - 1);
    c.len[FQ_LEN_ID * c.len_stride + r] = l_id;
    c.len[FQ_LEN_BASES * c.len_stride + r] = l_b;
    c.len[FQ_LEN_PLUS * c.len_stride + r] = l_p;
    c.len[FQ_LEN_QUAL * c.len_stride + r] = l_q;
    s_id += l_id; s_b += l_b; s_q += l_q;
    mx = l_id > mx ? l_id : mx;
    bad |= l_q != l_b ? 1u : 0u;
  }
  s_id = wave_sum32(s_id); s_b = wave_sum32(s_b); s_q = wave_sum32(s_q);
  mx = (u32)wave_max64(mx);
  bad = wave_any(bad != 0) ? 1u : 0u;
  if (FQ_LANE == 0) {
    u32 *o = red + FQ_WAVE_ID * 5;
    o[0] = s_id; o[1] = s_b; o[2] = s_q; o[3] = mx; o[4] = bad;
  }
  FQ_WG_BARRIER();
  if (FQ_T256 == 0) {
    u32 t[5] = {0, 0, 0, 0, 0};
    for (u32 w = 0; w < FQ_WAVES256; ++w) {
      const u32 *o = red + w * 5;
      t[0] += o[0]; t[1] += o[1]; t[2] += o[2];
      t[3] = o[3] > t[3] ? o[3] : t[3];
      t[4] |= o[4];
    }
    for (u32 k = 0; k < 5; ++k) c.rt[(u64)k * c.n_rtiles + FQ_BLOCK] = t[k];
  }
}

// one workgroup
FQ_KERNEL256 void k_fq_scan_rtiles(FqCfg c) {
  FQ_SHARED u32 ws[FQ_WAVES256];
  for (u32 q = 0; q < 3; ++q) {
    u64 run = 0;
    for (u32 b = 0; b < c.n_rtiles; b += FQ_N256) {
      const u32 i = b + FQ_T256;
      const u32 v = i < c.n_rtiles ? c.rt[(u64)q * c.n_rtiles + i] : 0u;
      u32 tot;
      const u32 ex = fq_wg_scan(wave_excl_scan32(v), wave_sum32(v), ws, tot);
      if (i < c.n_rtiles) c.rt_pre[(u64)q * (c.n_rtiles + 1) + i] = run + ex;
      run += tot;
    }
    if (FQ_T256 == 0) {
      c.rt_pre[(u64)q * (c.n_rtiles + 1) + c.n_rtiles] = run;
      c.summary[FQ_SUM_ID_BYTES + q] = run;
    }
  }
  u32 mx = 0, bad = 0;
  for (u32 i = FQ_T256; i < c.n_rtiles; i += FQ_N256) {
    const u32 m = c.rt[3ull * c.n_rtiles + i];
    mx = m > mx ? m : mx;
    bad |= c.rt[4ull * c.n_rtiles + i];
  }
  mx = (u32)wave_max64(mx);
  bad = wave_any(bad != 0) ? 1u : 0u;
  FQ_WG_BARRIER();
  if (FQ_LANE == 0) ws[FQ_WAVE_ID] = (mx << 1) | bad;   // (an id line is shorter than 2^31: chunks are below 4 GiB)
  FQ_WG_BARRIER();
  if (FQ_T256 == 0) {
    mx = 0; bad = 0;
    for (u32 w = 0; w < FQ_WAVES256; ++w) {
      mx = (ws[w] >> 1) > mx ? (ws[w] >> 1) : mx;
      bad |= ws[w] & 1u;
    }
    c.summary[FQ_SUM_RECORDS] = c.n_rec;
    c.summary[FQ_SUM_CONSUMED] = c.n_rec ? c.line_end[4 * c.n_rec - 1] + 1 : 0;
    c.summary[FQ_SUM_MAX_ID] = mx;
    c.summary[FQ_SUM_MISMATCH] = bad;
  }
}

FQ_KERNEL256 void k_fq_offsets(FqCfg c) {
  FQ_SHARED u32 ws[FQ_WAVES256];
  const u64 lo = (u64)FQ_BLOCK * FQSX_FQ_RTILE;
  for (u32 q = 0; q < 3; ++q) {
    const u32 *len = c.len + (u64)(q == 2 ? FQ_LEN_QUAL : q) * c.len_stride;
    u64 *off = c.off + (u64)q * c.off_stride;
    u64 run = c.rt_pre[(u64)q * (c.n_rtiles + 1) + FQ_BLOCK];
    for (u32 j0 = 0; j0 < FQSX_FQ_RTILE && lo + j0 < c.n_rec; j0 += FQ_N256) {
      const u64 r = lo + j0 + FQ_T256;
      const u32 v = r < c.n_rec ? len[r] : 0u;
      u32 tot;
      const u32 ex = fq_wg_scan(wave_excl_scan32(v), wave_sum32(v), ws, tot);
      if (r < c.n_rec) off[r] = run + ex;
      run += tot;
    }
    if (FQ_BLOCK + 1 == c.n_rtiles && FQ_T256 == 0) off[c.n_rec] = run;
  }
}

// A record's four lines lie side by side in the text: the lanes walk its bytes once and every byte goes to the column
// of the field it is in (the separator line and the line feeds of the base and quality lines go nowhere).
FQ_KERNEL256 void k_fq_gather(FqCfg c) {
  const u64 *id_off = c.off, *read_off = c.off + c.off_stride, *qual_off = c.off + 2 * c.off_stride;
  for (u32 b = uniform32(FQ_WAVE_ID); b < 4; b += FQ_WAVES256) {
    const u64 r0 = ((u64)FQ_BLOCK * 4 + b) * FQSX_FQ_GBATCH;
    for (u32 i = 0; i < FQSX_FQ_GBATCH && r0 + i < c.n_rec; ++i) {
      const u64 r = r0 + i;
      const u64 start = r ? c.line_end[4 * r - 1] + 1 : 0;
      const u64 e1 = c.line_end[4 * r], e2 = c.line_end[4 * r + 1], e3 = c.line_end[4 * r + 2], e4 = c.line_end[4 * r + 3];
      const u64 io = id_off[r], bo = read_off[r], qo = qual_off[r];
      // (what the passes before left is consistent by construction; checked all the same, so that nothing outside the
      // text and the columns is ever touched)
      if (!(start <= e1 && e1 < e2 && e2 < e3 && e3 < e4 && e4 < c.n)) continue;
      if (io + (e1 - start + 1) > c.col_n[0] || bo + (e2 - e1 - 1) > c.col_n[1] || qo + (e4 - e3 - 1) > c.col_n[2]) continue;
      for (u64 p = start + FQ_LANE; p < e4; p += FQ_WAVE) {
        const u8 ch = c.text[p];
        if (p <= e1) c.col[0][io + (p - start)] = ch;
        else if (p < e2) c.col[1][bo + (p - e1 - 1)] = ch;
        else if (p > e3) c.col[2][qo + (p - e3 - 1)] = ch;
      }
    }
  }
}
