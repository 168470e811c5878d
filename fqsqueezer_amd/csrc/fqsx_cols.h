// fqsx_cols.h -- a container block cut out of device-resident columns by read index.
//
// The FASTQ parser (fqsx_fastq.h) can leave the base and the quality column of every chunk it parses in device memory: one
// allocation per chunk that never moves, holding the chunk's own read offsets (n + 1, starting at 0), its bases and its
// qualities (one offset array serves both: a chunk whose quality lines differ in length from its base lines is refused).  A
// store is the table of those chunks; record r of the file is record r - rec0 of the last chunk whose rec0 is not above r.
//   k_cols_gather   read i of the block is record idx[i] of the store, or -- two stores, the mates of a paired file -- read 2i
//                   record idx[i] of the first and read 2i + 1 record idx[i] of the second.  The lanes of a wave look up one
//                   record each (index, chunk, source range, the block's own offsets) and check it; then the wave copies its
//                   records, sixteen lanes to a record, 16 bytes per lane where the destination is aligned.
// A record that fails a check sets its error word and is not copied, so nothing outside the block buffers is ever written;
// with store = 0 the kernel only checks, which is how the host refuses a block before a byte of the previous one is touched.
//   k_cols_locate   for the sort pre-pass of `-om s` (fqsx_sort.h), which reads the reads where the store keeps them: per record
//                   of the store the device address of its first base, its length and its bin, one record per lane, checked
//                   the same way.
// A store may keep the third column too (fqsx_cols_keep_ids): the id lines with their line feeds and offsets of their own,
// two more parts of every chunk's allocation.
//   k_cols_gather_ids   k_cols_gather for the id column: the same lookup and checks on the id offsets, one destination.
//   k_cols_id_survey    what the id coder's staging limits are compared with: over all records of the store the longest id
//                       line, the most tokens in a line, the longest instrument name and the most tokens up to a name's end;
//                       the lanes of a wave look up one record each, then sixteen lanes walk a line together.
// Workgroups are 256 threads (4 waves); the emulation build runs them as one 1-lane wave.
#pragma once
#include "fqsx_plat.h"
#include "fqsx_sort.h"

#ifndef FQSX_EMU
#define COLS_WAVES 4u   // waves of a workgroup
#define COLS_SUB 16u    // lanes that copy one record
#else
#define COLS_WAVES 1u
#define COLS_SUB 1u
#endif
enum { COLS_ERR_INDEX = 0, COLS_ERR_LENGTH = 1, COLS_ERR_RANGE = 2, COLS_N_ERR = 3 };

enum { COLS_READS = 0, COLS_IDS = 1 };   // the column a lookup is about: bases and qualities (one offset array), or the id lines
struct ColsChunk {
  const u8 *bases, *quals;   // [n_bytes] each
  const u64 *off;            // [n_rec + 1], off[0] = 0, off[n_rec] = n_bytes
  u64 rec0, n_rec, n_bytes;  // first record of the file in this chunk, its records and its bases
  const u8 *ids;             // [n_id_bytes] the id lines with their line feeds; null in a store that does not keep ids
  const u64 *id_off;         // [n_rec + 1], id_off[0] = 0, id_off[n_rec] = n_id_bytes
  u64 n_id_bytes;
};
struct ColsSrc {
  const ColsChunk *chunk;    // [n_chunks], rec0 ascending from 0
  u32 n_chunks;
  u64 n_rec;
};
struct ColsCfg {
  ColsSrc src[2];
  u32 n_src;        // 1, or 2: the reads of the block alternate between the two stores
  u32 store;        // 0: check only
  const u32 *idx;   // [n_out / n_src]
  const u64 *off;   // [n_out + 1]: the block's offsets
  u64 n_out;        // reads of the block
  u8 *out[2];       // bases, quals: [out_n] (k_cols_gather_ids: out[0] the id lines)
  u64 out_n;
  u32 *err;         // [COLS_N_ERR], nonzero: a record with an index beyond the store / whose length differs from the block's
                    // offsets / whose source or destination range is not inside its buffer
};

struct ColsRec { const u8 *sb, *sq; u64 d; u32 len; };   // source of the bases and of the qualities, destination offset, bytes
struct alignas(16) Cols16 { u64 lo, hi; };

// the last of the n_chunks > 0 chunks whose rec0 is not above rec
FQ_DEV u32 cols_chunk_of(const ColsChunk *chunk, u32 n_chunks, u64 rec) {
  u32 lo = 0, hi = n_chunks;   // chunk[lo].rec0 <= rec < chunk[hi].rec0
  while (hi - lo > 1) {
    const u32 mid = lo + (hi - lo) / 2;
    if (chunk[mid].rec0 <= rec) lo = mid; else hi = mid;
  }
  return lo;
}

// record rec of a store, rec < src.n_rec: where column col of it lies (sq: its qualities, reads only) and its bytes; false
// -- a device error -- if the chunk table or the chunk's offsets do not hold it
FQ_DEV bool cols_source(const ColsChunk *chunk, u32 n_chunks, u32 col, u64 rec, const u8 *&sb, const u8 *&sq, u32 &len) {
  if (n_chunks == 0) return false;
  const ColsChunk ch = chunk[cols_chunk_of(chunk, n_chunks, rec)];
  if (rec < ch.rec0 || rec - ch.rec0 >= ch.n_rec) return false;
  const u64 *off = col == COLS_IDS ? ch.id_off : ch.off;
  const u64 n_bytes = col == COLS_IDS ? ch.n_id_bytes : ch.n_bytes;
  if (col == COLS_IDS && (!ch.ids || !off)) return false;
  const u64 so = off[rec - ch.rec0], se = off[rec - ch.rec0 + 1];
  if (se < so || se > n_bytes || se - so > 0xffffffffull) return false;
  sb = (col == COLS_IDS ? ch.ids : ch.bases) + so;
  sq = col == COLS_IDS ? nullptr : ch.quals + so;
  len = (u32)(se - so);
  return true;
}

// read i of the block in column col: where it comes from and where it goes, len = 0 unless every check passes
FQ_DEV ColsRec cols_lookup(const ColsCfg &c, u32 col, u64 i) {
  ColsRec r = {nullptr, nullptr, 0, 0};
  if (i >= c.n_out) return r;
  const bool second = c.n_src == 2 && (i & 1);
  const ColsChunk *chunk = second ? c.src[1].chunk : c.src[0].chunk;
  const u32 n_chunks = second ? c.src[1].n_chunks : c.src[0].n_chunks;
  const u64 n_rec = second ? c.src[1].n_rec : c.src[0].n_rec;
  const u64 rec = c.idx[c.n_src == 2 ? i >> 1 : i];
  if (rec >= n_rec) { c.err[COLS_ERR_INDEX] = 1; return r; }
  const u8 *sb = nullptr, *sq = nullptr;
  u32 len = 0;
  if (!cols_source(chunk, n_chunks, col, rec, sb, sq, len)) { c.err[COLS_ERR_RANGE] = 1; return r; }
  const u64 d0 = c.off[i], d1 = c.off[i + 1];
  if (d1 < d0 || d1 - d0 != len) { c.err[COLS_ERR_LENGTH] = 1; return r; }
  if (d1 > c.out_n) { c.err[COLS_ERR_RANGE] = 1; return r; }
  r.sb = sb; r.sq = sq; r.d = d0; r.len = len;
  return r;
}

// len bytes from src to dst by the COLS_SUB lanes of a record (sl: this lane among them): source and destination are aligned
// to nothing, so bytes up to the destination's first 16-byte boundary, 16-byte groups (loads from wherever the source
// happens to lie, aligned stores), then the bytes that are left
FQ_DEV void cols_copy(u8 *dst, const u8 *src, u32 len, u32 sl) {
  const u32 to_boundary = (u32)((16u - ((u64)(uintptr_t)dst & 15u)) & 15u), head = to_boundary < len ? to_boundary : len;
  const u32 groups = (len - head) / 16u, tail = head + 16u * groups;
  for (u32 p = sl; p < head; p += COLS_SUB) dst[p] = src[p];
  for (u32 g = sl; g < groups; g += COLS_SUB) {
    Cols16 v;
    __builtin_memcpy(&v, src + head + 16u * g, 16);
    *(Cols16 *)(dst + head + 16u * g) = v;
  }
  for (u32 p = tail + sl; p < len; p += COLS_SUB) dst[p] = src[p];
}

FQ_KERNEL256 void k_cols_gather(ColsCfg c) {
  const u64 i0 = ((u64)FQ_BLOCK * COLS_WAVES + FQ_WAVE_ID) * FQ_WAVE;
  const ColsRec mine = cols_lookup(c, COLS_READS, i0 + FQ_LANE);
  if (!c.store) return;
  for (u32 j0 = 0; j0 < FQ_WAVE; j0 += FQ_WAVE / COLS_SUB) {
    const u32 from = j0 + FQ_LANE / COLS_SUB, sl = FQ_LANE % COLS_SUB;
    const u32 len = wave_bcast32(mine.len, from);
    const u64 d = wave_bcast64(mine.d, from);
    const u8 *sb = (const u8 *)(uintptr_t)wave_bcast64((u64)(uintptr_t)mine.sb, from);
    const u8 *sq = (const u8 *)(uintptr_t)wave_bcast64((u64)(uintptr_t)mine.sq, from);
    if (len == 0) continue;
    cols_copy(c.out[0] + d, sb, len, sl);
    cols_copy(c.out[1] + d, sq, len, sl);
  }
}

FQ_KERNEL256 void k_cols_gather_ids(ColsCfg c) {
  const u64 i0 = ((u64)FQ_BLOCK * COLS_WAVES + FQ_WAVE_ID) * FQ_WAVE;
  const ColsRec mine = cols_lookup(c, COLS_IDS, i0 + FQ_LANE);
  if (!c.store) return;
  for (u32 j0 = 0; j0 < FQ_WAVE; j0 += FQ_WAVE / COLS_SUB) {
    const u32 from = j0 + FQ_LANE / COLS_SUB, sl = FQ_LANE % COLS_SUB;
    const u32 len = wave_bcast32(mine.len, from);
    const u64 d = wave_bcast64(mine.d, from);
    const u8 *sb = (const u8 *)(uintptr_t)wave_bcast64((u64)(uintptr_t)mine.sb, from);
    if (len == 0) continue;
    cols_copy(c.out[0] + d, sb, len, sl);
  }
}

// Where the sort pre-pass finds record r, and the reference's bin of it: the first four bases under A, C, G = 0, 1, 2 and
// everything else 3 -- a position past the end of the read included, which there lands on the line feed (preprocess_se,
// application.cpp:383-391).  (The sort KEY of a missing position is 0, sort_digit: "shorter first".  Both rules meet in reads
// of fewer than four bases.)  A record that fails a check sets the error word and is written as an empty read at address 0.
struct ColsLocCfg {
  ColsSrc src;
  u64 *addr;   // [src.n_rec] device address of the record's first base
  u32 *len;    // [src.n_rec]
  u8 *bin;     // [src.n_rec]
  u32 *err;    // [COLS_N_ERR]
};
FQ_KERNEL256 void k_cols_locate(ColsLocCfg c) {
  const u64 r = ((u64)FQ_BLOCK * COLS_WAVES + FQ_WAVE_ID) * FQ_WAVE + FQ_LANE;
  if (r >= c.src.n_rec) return;
  const u8 *p = nullptr, *q = nullptr;
  u32 len = 0;
  const bool ok = cols_source(c.src.chunk, c.src.n_chunks, COLS_READS, r, p, q, len);
  if (!ok) c.err[COLS_ERR_RANGE] = 1;
  u32 id = 0;
  for (u32 i = 0; i < 4; ++i) id = (id << 2) | (i < len ? sort_nt(p[i]) : 3u);
  c.addr[r] = (u64)(uintptr_t)p;
  c.len[r] = len;
  c.bin[r] = (u8)id;
}

// The id lines of a store against the id kernel's staging limits (fqsx_idk.h; the comparison is the caller's).  Per line, with
// its line feed: its bytes; its tokens, the bytes outside [0-9A-Za-z@] (idk_is_lit); and -- a line with a '.', ' ' or ':' has an
// instrument name in front of the first of them -- the name's bytes, cut short at a NUL, and the tokens up to the name's end
// plus the terminator the name is coded with.  The maxima of the four are reduced over the lanes of a record, the wave and the
// workgroup (LDS); thread 0 stores the workgroup's four words, which the host reduces: no atomics.
enum { COLS_SV_LINE = 0, COLS_SV_TOKENS = 1, COLS_SV_NAME = 2, COLS_SV_NAME_TOKENS = 3, COLS_N_SV = 4 };
struct ColsSurveyCfg {
  ColsSrc src;
  u32 *part;   // [groups][COLS_N_SV]
  u32 *err;    // [COLS_N_ERR]
};
FQ_DEV bool cols_id_is_lit(u8 c) { return (c >= '0' && c <= '9') || (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || c == '@'; }
// over the COLS_SUB lanes of a record (aligned groups of lanes: the butterfly stays inside them)
FQ_DEV u32 cols_sub_sum(u32 v) {
  for (u32 o = COLS_SUB / 2; o > 0; o >>= 1) v += wave_xor32(v, o);
  return v;
}
FQ_DEV u32 cols_sub_min(u32 v) {
  for (u32 o = COLS_SUB / 2; o > 0; o >>= 1) {
    const u32 y = wave_xor32(v, o);
    v = y < v ? y : v;
  }
  return v;
}
FQ_KERNEL256 void k_cols_id_survey(ColsSurveyCfg c) {
  FQ_SHARED u32 red[COLS_WAVES * COLS_N_SV];
  const u64 r = ((u64)FQ_BLOCK * COLS_WAVES + FQ_WAVE_ID) * FQ_WAVE + FQ_LANE;
  const u8 *mine = nullptr, *none = nullptr;
  u32 mine_len = 0;
  if (r < c.src.n_rec && !cols_source(c.src.chunk, c.src.n_chunks, COLS_IDS, r, mine, none, mine_len)) {
    c.err[COLS_ERR_RANGE] = 1;
    mine_len = 0;
  }
  u32 mx[COLS_N_SV] = {0, 0, 0, 0};
  for (u32 j0 = 0; j0 < FQ_WAVE; j0 += FQ_WAVE / COLS_SUB) {
    const u32 from = j0 + FQ_LANE / COLS_SUB, sl = FQ_LANE % COLS_SUB;
    const u32 len = wave_bcast32(mine_len, from);
    const u8 *p = (const u8 *)(uintptr_t)wave_bcast64((u64)(uintptr_t)mine, from);
    // (len is the same in the lanes of a record, so they stay together through the reductions below)
    u32 seps = 0, end = len, nul = len;   // tokens of the line; its first '.', ' ' or ':'; its first NUL
    for (u32 k = sl; k < len; k += COLS_SUB) {
      const u8 ch = p[k];
      seps += cols_id_is_lit(ch) ? 0u : 1u;
      if ((ch == '.' || ch == ' ' || ch == ':') && k < end) end = k;
      if (ch == 0 && k < nul) nul = k;
    }
    seps = cols_sub_sum(seps); end = cols_sub_min(end); nul = cols_sub_min(nul);
    mx[COLS_SV_LINE] = len > mx[COLS_SV_LINE] ? len : mx[COLS_SV_LINE];
    mx[COLS_SV_TOKENS] = seps > mx[COLS_SV_TOKENS] ? seps : mx[COLS_SV_TOKENS];
    if (end < len) {   // a line with a name: [0, end), cut short at a NUL
      u32 before = 0;
      for (u32 k = sl; k < end; k += COLS_SUB) before += cols_id_is_lit(p[k]) ? 0u : 1u;
      before = cols_sub_sum(before) + 1u;
      const u32 name = nul < end ? nul : end;
      mx[COLS_SV_NAME] = name > mx[COLS_SV_NAME] ? name : mx[COLS_SV_NAME];
      mx[COLS_SV_NAME_TOKENS] = before > mx[COLS_SV_NAME_TOKENS] ? before : mx[COLS_SV_NAME_TOKENS];
    }
  }
  for (u32 k = 0; k < COLS_N_SV; ++k) mx[k] = (u32)wave_max64(mx[k]);
  if (FQ_LANE == 0)
    for (u32 k = 0; k < COLS_N_SV; ++k) red[FQ_WAVE_ID * COLS_N_SV + k] = mx[k];
  FQ_WG_BARRIER();
  if (FQ_WAVE_ID == 0 && FQ_LANE == 0) {
    for (u32 k = 0; k < COLS_N_SV; ++k) {
      u32 m = 0;
      for (u32 w = 0; w < COLS_WAVES; ++w) m = red[w * COLS_N_SV + k] > m ? red[w * COLS_N_SV + k] : m;
      c.part[(u64)FQ_BLOCK * COLS_N_SV + k] = m;
    }
  }
}
