/* fqsx.h -- C ABI of the MI355X-native FQSqueezer DNA path (libfqsx.so).
 *
 * The reference (refresh-bio/fqsqueezer v1.1) has no plugin/FFI surface; the narrowest
 * seam its DNA hot path sits behind is the public interface of CDNACompressor as driven by
 * the worker lambda of CApplication::compress_se_files.  This ABI replaces that seam at
 * *reads-block* granularity:
 *
 *   fqsx_dna_create        <- CDNACompressor::SetParams/SetCoder/Init/SetKmerDS for all T
 *                             workers + CApplication::AdjustToParams
 *                             (fqs/compressor.h:42-43, fqs/dna.h:263-269,
 *                              fqs/application.cpp:77-108, :578-608)
 *   fqsx_dna_encode_block  <- one iteration of the worker loop for all T workers:
 *                             ResetReadPrev, Start, CompressDirect|CompressSorted per read,
 *                             the barrier-synchronised InsertKmersToHT/ClearKmersToHT
 *                             phases, End  (fqs/application.cpp:610-669, fqs/dna.h:271-285)
 *   fqsx_dna_destroy       <- ~CDNACompressor / ~CApplication
 *
 * The library is HIP-only: it fails with FQSX_E_NO_DEVICE when no gfx950 GPU is present.
 * There is no CPU code path behind this ABI.
 *
 * Threading: one fqsx_dna per output file, calls serialised by the caller, blocks in file
 * order (models persist across blocks exactly like the reference's per-thread compressors).
 */
#ifndef FQSX_H
#define FQSX_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct fqsx_dna fqsx_dna;

/* Transport of the sharded mode: the collectives among the `world` ranks (one process per GPU) that share one file, on
 * buffers in the codec's memory space (device memory).  fqsx_rccl_comm_create gives the RCCL one (xGMI inside a node);
 * a caller with a transport of its own (MPI, a test harness) fills in the three functions.  Each returns 0 on success
 * and may return before the operation has completed as long as later work on the codec's stream waits for it. */
typedef struct fqsx_comm {
  void *ctx;
  /* in-place sum over the ranks of n 32-bit words */
  int (*allreduce_sum_u32)(void *ctx, uint32_t *buf, uint64_t n);
  /* n_buf variable all-to-alls of 64-bit words in one go: buffer b sends send_counts[b * world + r] words to rank r (the
   * parts lie back to back in send[b], in rank order) and receives recv_counts[b * world + q] words from rank q likewise */
  int (*alltoallv_u64)(void *ctx, uint32_t n_buf, const uint64_t *const *send, const uint64_t *send_counts,
                       uint64_t *const *recv, const uint64_t *recv_counts);
  /* every rank contributes n 64-bit words; recv = [world][n] */
  int (*allgather_u64)(void *ctx, const uint64_t *send, uint64_t n, uint64_t *recv);
  /* optional (may be null): give the transport up after a failed collective, so that this rank's part of whatever is still
   * pending does not keep the other ranks waiting (RCCL: ncclCommAbort) */
  void (*abort)(void *ctx);
} fqsx_comm;

enum {
  FQSX_OK = 0,
  FQSX_E_ARG = -1,        /* bad argument / malformed header / unsupported dna_mode */
  FQSX_E_NO_DEVICE = -2,  /* no HIP device (the library has no CPU fallback) */
  FQSX_E_HIP = -3,        /* HIP runtime error, see fqsx_last_error() */
  FQSX_E_NOMEM = -4,      /* device allocation failed */
  FQSX_E_DEVICE = -5,     /* device-side error word set (table/stream overflow) */
  FQSX_E_PEER = -6        /* sharded mode: another rank of the world failed; every rank has left the phase (this one was fine) */
};

/* header17: the 17 parameter bytes of the .fqs file being written
 * ('K','C','S','D', no_threads T, dna_mode, quality_mode, id_mode, quality_thr,
 *  duplicates_check, prefix_len, pmer_len, smer_len, bmer_len, imer_len, hmer_len,
 *  ht_prefix_len; fqs/params.h:80-100).  T is the number of logical workers and is part of
 * the bitstream.  dna_mode 0..3 (se_original, se_sorted, pe_original, pe_sorted) are implemented; in the
 * paired modes a block holds the mates interleaved (mate 1, mate 2, mate 1, ...) and n_reads is even.
 * device: HIP device ordinal. */
int fqsx_dna_create(const uint8_t *header17, int device, fqsx_dna **out);
/* The same with the codec's kernels confined to compute units [part * CUs / n_parts, (part + 1) * CUs / n_parts) of the
 * device (a HIP stream with a CU mask).  One file with T <= 64 workers occupies T of the 256 CUs (a worker's workgroup
 * takes a whole CU's LDS), so a GPU has room for several files; giving every concurrent file a partition of its own keeps
 * their kernels from queueing behind each other for compute units.  n_parts = 1: the whole device (= fqsx_dna_create). */
int fqsx_dna_create_on_partition(const uint8_t *header17, int device, uint32_t part, uint32_t n_parts, fqsx_dna **out);
void fqsx_dna_destroy(fqsx_dna *);

/* Encode one reads block.  bases = concatenated ASCII sequences (ACGTN) of the block's
 * reads in block order, read_off = n_reads+1 byte offsets into bases (host memory).
 * generation = index of the block within the file (drives the synchronisation schedule,
 * fqs/application.h:85-92).  On return streams[w]/lens[w] (w < T) describe worker w's
 * complete DNA range-coder stream for this block in host memory owned by the codec and
 * valid until the next call on the same codec. */
int fqsx_dna_encode_block(fqsx_dna *, const uint8_t *bases, const uint64_t *read_off, uint32_t n_reads,
                          uint32_t generation, const uint8_t **streams, uint64_t *lens);

/* Same with the block already resident in device memory (HBM): d_bases / d_read_off are
 * device pointers; h_read_off is the host copy of the offsets (needed for sizing). */
int fqsx_dna_encode_block_dev(fqsx_dna *, const uint8_t *d_bases, const uint64_t *d_read_off,
                              const uint64_t *h_read_off, uint32_t n_reads, uint32_t generation,
                              const uint8_t **streams, uint64_t *lens);

/* Decode one reads block: inverse of fqsx_dna_encode_block (replaces one generation of the reference's
 * decoder workers, fqs/application.cpp:874-917 with CDNACompressor::DecompressSE / DecompressPE,
 * fqs/dna.h:277-278).  streams[w]/lens[w] = worker w's DNA stream of the block (host memory), read_off =
 * n_reads+1 offsets of the reads inside bases_out (the read lengths come from the meta stream).  A codec
 * instance is used either for encoding or for decoding a file, never both.
 * Refused with FQSX_E_ARG before anything is launched, the codec unchanged: offsets that do not start at 0 or descend, a read of
 * 2^24 bases or more, an odd n_reads in a paired mode, a null stream with a length.
 * A stream that leaves the format ("Where a DNA stream leaves the format") or runs a table or mailbox over:
 * FQSX_E_DEVICE ("device error 8 in decode kernel" for the former); nothing outside bases_out[0 .. read_off[n_reads]) is written
 * and the call returns.  A damaged stream can also decode to bases without an error: the range decoder has no check sum.
 * After FQSX_E_DEVICE the codec's tables, models and contexts are partly updated with what the block decoded up to the error:
 * the only call that may follow on it is fqsx_dna_destroy, and the file is decoded again from its first block with a new codec. */
int fqsx_dna_decode_block(fqsx_dna *, const uint8_t *const *streams, const uint64_t *lens, const uint64_t *read_off,
                          uint32_t n_reads, uint32_t generation, uint8_t *bases_out);

/* The same, leaving the block in device memory: *d_bases_out is the codec's own output buffer, valid until the next call on
 * the codec; null on error.  The call returns with the codec's stream drained, so another stream may read the block. */
int fqsx_dna_decode_block_dev(fqsx_dna *, const uint8_t *const *streams, const uint64_t *lens, const uint64_t *read_off,
                              uint32_t n_reads, uint32_t generation, const uint8_t **d_bases_out);

/* Accounting counters summed over workers since creation:
 * [0] global probes [1] global slots read [2] local probes [3] local slots read
 * [4] global inserts [5] slots read by them [6] siv words touched [7] context slots read
 * [8] symbols range-coded [9] local inserts [10] mailbox entries [11] input bases
 * [12] siv words of the reference's rank sweeps (fqs/dna.cpp:600-605) that the count index spared the kernels ([6] + [12] = the
 *      words the algorithm sweeps)
 * [13] decoder: b-mer look-ups whose buckets, requested a position ahead, belonged to another k-mer after a revert and were looked up again
 * [16..63] in-kernel section timers / event counts (10 ns ticks, only in -DFQSX_TIMING diagnostic builds) */
int fqsx_dna_stats(fqsx_dna *, uint64_t out[64]);

/* Table occupancy and device memory (no counterpart in the reference, which prints table populations at -v 2,
 * fqs/application.cpp:733-741): [0] distinct s-mers stored [1] distinct b-mers stored [2] s-mer table slots (all owners)
 * [3] b-mer table slots [4] p-mer vector bytes [5] context-table slots (all workers) [6] contexts stored
 * [7] device bytes held now [8] ... at most so far (old + new table during a growth included) [9] table growth events
 * [10] minimizer pairs stored (paired-end) [11] pair-table slots (16 bytes each) [12] bytes per k-mer table slot
 * [13] bytes of s- + b-mer table memory this rank holds (all of it, or its owners' share with partitioned tables)
 * [14] bytes of pair-table memory this rank holds (likewise) [15] bytes of the p-mer vector this rank holds (likewise). */
int fqsx_dna_capacity(fqsx_dna *, uint64_t out[16]);

/* One GPU's capacity mode (no counterpart in the reference, whose sub-tables are separate heap vectors that grow one by one,
 * fqs/ht_kmer.h:88-112): before the first block, switch the s- and b-mer tables to one chunk of physical memory per
 * sub-table inside one reserved address range (HIP virtual-memory API).  The kernels see the same layout; a growth then
 * re-inserts sub-table by sub-table and returns each old chunk before the next new one is made, so the peak is the new table
 * plus one old sub-table instead of old + new side by side.  Also chosen by the environment variable FQSX_CHUNKED_TABLES=1; and a
 * table that reaches 2 GiB (FQSX_CHUNK_AUTO_KB: another size in KiB, 0 = never) turns into a chunked table at that growth by itself. */
int fqsx_dna_use_chunked_tables(fqsx_dna *);

/* Sharded mode (reference: the T x T mailboxes of fqs/application.h:56-59 and their owner-side
 * application, fqs/dna.cpp:825-847, :2393-2472): logical worker w -- coder state, RNG streams, local tables and the
 * sub-tables it owns -- lives on rank w % world; every rank keeps a replica of all sub-tables for the look-ups (or maps the
 * other ranks' sub-tables: fqsx_shard_partition_tables below).  The streams are bit-identical to the one-GPU run's.
 * There is one driver, the phase loop inside the library (the reference's phase is three barrier waits,
 * fqs/application.cpp:643-655): fqsx_shard_attach makes the codec one rank of the world and hands it the transport (the world's
 * collectives, fqsx_comm); fqsx_shard_encode_block runs a whole reads block -- per phase three
 * collectives (all-reduce of the count matrix; the three mailboxes in one grouped all-to-all; one all-gather carrying the
 * applied items, the p-mer statistics and, paired-end, the pair-table triples) and one host round trip (transfer sizes,
 * table demand, error word).  All four dna_modes.  bases / read_off: the block in the codec's memory space, the same on
 * every rank; streams[w] / lens[w] are meaningful for this rank's workers (w % world == rank).
 * fqsx_shard_traffic: [0] phases [1] collectives issued [2] all-to-all words sent to other ranks [3] all-gather words sent. */
int fqsx_shard_attach(fqsx_dna *, uint32_t rank, uint32_t world, const fqsx_comm *comm);
int fqsx_shard_encode_block(fqsx_dna *, const uint8_t *bases /*[codec]*/, const uint64_t *read_off /*[codec]*/, const uint64_t *h_read_off,
                            uint32_t n_reads, uint32_t generation, const uint8_t **streams, uint64_t *lens);
int fqsx_shard_traffic(fqsx_dna *, uint64_t out[4]);
/* Partitioned look-ups (SURVEY.md 8e option (i); the reference shares ONE table among its threads, fqs/application.h:51-54,
 * with the owner functions of fqs/dna.cpp:825 and :2381-2386 deciding who writes a key).  Collective over the ranks of one
 * node, after fqsx_shard_attach and before the first block: from then on a rank holds the physical memory of only the s- and
 * b-mer sub-tables its workers own (1/world of the k-mer tables) and maps the other ranks' sub-tables beside them
 * (hipMemCreate -> POSIX descriptor over a Unix socket -> hipMemImportFromShareableHandle -> hipMemMap), so that every rank
 * sees one table in one address range and a look-up of a foreign sub-table is a load over xGMI.  Writes stay with the owner
 * (insert phase); the phase's collectives order them before the next look-ups.  The all-gather of a phase then carries no
 * k-mer items, only the owners' occupancy counters, the p-mer items and statistics and the paired-end triples.  The p-mer
 * vector (fqs/application.h:51 siv_pmer, owner function fqs/dna.cpp:658) is partitioned as well when its 4096 owner ranges
 * reach the chunk granule (2 MiB: the 16 GiB vector of the default geometry; smaller vectors stay replicas): a range lives on
 * its owner's rank, the count index over the vector stays a replica that follows the owners' log of changed fields.  A paired-end codec's pair table (fqs/application.h:54 ht_pe_mers, owner function
 * fqs/ht_kmer.h:599-602) is partitioned the same way: every rank receives every source's triples but applies those of its
 * own owners only, and a fourth one-word all-reduce closes such a phase (the inserts follow the phase's last collective).
 * Streams are bit-identical to the one-GPU run's.
 * Memory order: the kernels that write own sub-tables (insert phase, growth) end with a system-scope release and the encode /
 * decode kernels start behind a system-scope acquire (csrc/fqsx_plat.h), so that an owner's writes are in its HBM before the
 * phase's last collective and no GPU serves a foreign look-up from a line it cached in an earlier launch.
 * Peer access: the ranks all-gather their GPUs' PCI bus ids and ask hipDeviceCanAccessPeer; if any pair of the world cannot
 * reach each other ALL ranks stay with table replicas -- the call still returns FQSX_OK, fqsx_last_error() says why and
 * fqsx_shard_is_partitioned() returns 0.
 * fqsx_dna_capacity()[13] = bytes of k-mer table memory this rank holds. */
int fqsx_shard_partition_tables(fqsx_dna *);
int fqsx_shard_is_partitioned(fqsx_dna *);
/* RCCL transport on the codec's own stream (collectives and kernels are ordered by the stream; librccl is loaded on first
 * use).  Rank 0 calls fqsx_rccl_unique_id and hands the 128 bytes to the other ranks by any means (a file, a TCP store). */
int fqsx_rccl_unique_id(uint8_t id[128]);
int fqsx_rccl_comm_create(fqsx_dna *, const uint8_t id[128], uint32_t rank, uint32_t world, fqsx_comm *out);
/* The communicator goes on with another codec (the next file of the process): its collectives run on that codec's stream. */
int fqsx_rccl_comm_rebind(fqsx_comm *, fqsx_dna *);
/* out[0] = ranks of the communicator as RCCL counts them (ncclCommCount), out[1] = this process's rank in it. */
int fqsx_rccl_comm_info(fqsx_comm *, uint32_t out[2]);
void fqsx_rccl_comm_destroy(fqsx_comm *);

/* Kernel timing: when enabled every launch is bracketed by HIP events on the codec's stream.
 * out[0..2] = accumulated milliseconds of the encode-segment, insert-phase and all other
 * kernels; out[3..5] = their launch counts. */
int fqsx_dna_set_profiling(fqsx_dna *, int enable);
int fqsx_dna_kernel_times(fqsx_dna *, double out[6]);
/* Diagnostic builds (-DFQSX_TIMING) only: per-launch, per-worker clock stamps of the five roles of the encode kernel,
 * out[launch][worker][FQSX_TRACE_WORDS]: 8 stamps in 10 ns ticks + 24 per-launch counters / section times of the resolving wave; returns the
 * number of launches copied (always 0 in the product build).  `out` must hold max_launches * T * FQSX_TRACE_WORDS words. */
#define FQSX_TRACE_WORDS 32
int fqsx_dna_trace(fqsx_dna *, uint64_t *out, uint32_t max_launches);

/* Quality stream on the GPU: replaces CQualityCompressor::Init / Compress for all T
 * workers of a block (fqs/quality.h:43-50, fqs/quality.cpp:32-71,152-175; called from fqs/application.cpp:641).
 * quality_mode and quality_thr come from the header bytes 6 and 8; quality_mode none is rejected (nothing
 * to code).  quals = concatenated quality strings of the block's reads (mates interleaved for paired data). */
typedef struct fqsx_qual fqsx_qual;
int fqsx_qual_create(const uint8_t *header17, int device, fqsx_qual **out);
int fqsx_qual_encode_block(fqsx_qual *, const uint8_t *quals, const uint64_t *read_off, uint32_t n_reads,
                           const uint8_t **streams, uint64_t *lens);
/* Same with the block already resident in device memory (d_quals / d_read_off device pointers, h_read_off the host copy). */
int fqsx_qual_encode_block_dev(fqsx_qual *, const uint8_t *d_quals, const uint64_t *d_read_off, const uint64_t *h_read_off,
                               uint32_t n_reads, const uint8_t **streams, uint64_t *lens);
/* Decode one block's quality stream: inverse of fqsx_qual_encode_block (replaces CQualityCompressor::Decompress for all T
 * workers, fqs/quality.cpp:175-200 with CRangeCoderModel::Decode, fqs/rc.h:403-421, and CRangeDecoder, fqs/sub_rc.h:93-158;
 * called from the decoder workers, fqs/application.cpp:874-917).  streams[w] / lens[w] = worker w's quality stream of the
 * block (host memory), read_off = n_reads+1 offsets of the reads inside quals_out, starting at 0 (the read lengths come from
 * the meta stream).  quals_out receives the ASCII qualities (quality_code_map_rev + 33).  A worker that has symbols to
 * decode and a stream shorter than 8 bytes: FQSX_E_ARG; a stream whose cumulative frequency leaves its model (malformed):
 * FQSX_E_DEVICE, nothing outside read_off's range is written.  A codec instance is used either for encoding or for decoding
 * a file, never both. */
int fqsx_qual_decode_block(fqsx_qual *, const uint8_t *const *streams, const uint64_t *lens, const uint64_t *read_off,
                           uint32_t n_reads, uint8_t *quals_out);
/* The same, leaving the block in device memory: *d_quals_out is owned by the codec and valid until the next call. */
int fqsx_qual_decode_block_dev(fqsx_qual *, const uint8_t *const *streams, const uint64_t *lens, const uint64_t *read_off,
                               uint32_t n_reads, const uint8_t **d_quals_out);
/* Contexts stored per worker (out[0..T)) and, in out[T], the slots per worker of the context table (the reference's
 * m_ctx_rc, fqs/quality.h:30): what a decoder must agree on with the encoder of the same data. */
int fqsx_qual_contexts(fqsx_qual *, uint64_t *out);
int fqsx_qual_set_profiling(fqsx_qual *, int enable);         /* HIP events around every launch of the quality kernel (encode or decode) ... */
int fqsx_qual_kernel_times(fqsx_qual *, double out[2]);       /* ... out[0] = accumulated milliseconds, out[1] = launches */
void fqsx_qual_destroy(fqsx_qual *);

/* Host-side (CPU) read-length stream that accompanies every DNA stream in the container
 * (CMetaCompressor::CompressReadLen, fqs/meta.cpp:48-113; one symbol per read, not part of the hot path).
 * Same worker partition as the DNA path; streams valid until the next call. */
typedef struct fqsx_meta fqsx_meta;
int fqsx_meta_create(uint32_t T, fqsx_meta **out);
int fqsx_meta_encode_block(fqsx_meta *, const uint32_t *read_len, uint32_t n_reads, const uint8_t **streams,
                           uint64_t *lens);
/* paired != 0: reads alternate mate 1 / mate 2 (CompressReadLenPE, fqs/meta.cpp:100-107) */
int fqsx_meta_encode_block_pe(fqsx_meta *, const uint32_t *read_len, uint32_t n_reads, int paired,
                              const uint8_t **streams, uint64_t *lens);
/* Inverse of fqsx_meta_encode_block_pe (CMetaCompressor::DecompressReadLen / DecompressReadLenPE, fqs/meta.cpp:76-131):
 * n_reads comes from the container block's header, paired as in the encoder.  A stream that runs out of bytes or is
 * malformed: FQSX_E_ARG.  An instance is used either for encoding or for decoding a file, never both. */
int fqsx_meta_decode_block(fqsx_meta *, const uint8_t *const *streams, const uint64_t *lens, uint32_t n_reads, int paired,
                           uint32_t *read_len_out);
void fqsx_meta_destroy(fqsx_meta *);

/* Read-id stream (host CPU by design: string tokeniser + delta coder).  Replaces
 * CIdCompressor::Init / ResetReadPrev / Compress / CompressPE for all T workers of one block (fqs/id.h:152-164,
 * id.cpp:138-184; application.cpp:600-601,625,635,1165).  header17: T = byte 4, id_mode = byte 7 (0 lossless,
 * 1 instrument, 2 none).  ids = concatenated id lines each including its '\n'; id_off = n_reads+1 offsets;
 * paired != 0: reads alternate mate 1 / mate 2.  Streams are callee-owned until the next call.
 * FQSX_E_ARG for bytes >= 128 in an id (the reference indexes 128-symbol models with them) and, in instrument
 * mode, for an id without any of '.', ' ', ':' (the reference then overwrites the first base). */
typedef struct fqsx_id fqsx_id;
int fqsx_id_create(const uint8_t *header17, fqsx_id **out);
int fqsx_id_encode_block(fqsx_id *, const uint8_t *ids, const uint64_t *id_off, uint32_t n_reads, int paired,
                         const uint8_t **streams, uint64_t *lens);
void fqsx_id_destroy(fqsx_id *);

/* The read-id stream on the GPU: same arguments and the same bytes as fqsx_id_encode_block, coded by one
 * wavefront per worker (csrc/fqsx_idk.h: tokeniser, numeric deltas, move-to-front list of instrument names, adaptive models in
 * per-worker tables in HBM; reference fqs/id.cpp:152-184, 257-495, 734-757).  Staging limits of the kernel: id lines of at most
 * 1024 bytes with the line feed, 128 tokens (every byte outside [0-9A-Za-z@] ends one, the line feed included), instrument names
 * of 62 bytes, 4096 distinct instrument names per worker (beyond: FQSX_E_DEVICE with fqsx_idg_error_kind 5 or 6, use the host
 * coder: it writes the same bytes, so a file can change over between two blocks).  id_mode none has no stream. */
typedef struct fqsx_idg fqsx_idg;
int fqsx_idg_create(const uint8_t *header17, int device, fqsx_idg **out);
int fqsx_idg_encode_block(fqsx_idg *, const uint8_t *ids, const uint64_t *id_off, uint32_t n_reads, int paired,
                          const uint8_t **streams, uint64_t *lens);
/* fqsx_idg_encode_block for a block that lies in device memory, as fqsx_cols_gather_ids leaves it: d_ids = the id lines back to
 * back in a buffer with 64 spare bytes behind them, d_id_off = their n_reads + 1 offsets there, h_id_off = the same offsets on
 * the host.  The same streams, errors, fqsx_idg_error_kind and table sizes (fqsx_idg_stats [4], [5]) as fqsx_idg_encode_block
 * on the same ids: what that call counts on the host to size its model tables, the separators of every worker's lines, a
 * kernel counts here (one workgroup per worker, one transfer of T counts).  Everything runs on the codec's stream: the caller
 * guarantees that the stream that wrote the buffers is drained (fqsx_cols_gather_ids returns so) and keeps them until the call
 * returns.  fqsx_idg_separator_times (after fqsx_idg_set_profiling): out[0] / out[1] milliseconds and launches of that kernel. */
int fqsx_idg_encode_block_dev(fqsx_idg *, const uint8_t *d_ids, const uint64_t *d_id_off, const uint64_t *h_id_off, uint32_t n_reads,
                              int paired, const uint8_t **streams, uint64_t *lens);
void fqsx_idg_destroy(fqsx_idg *);

/* Decode one block's id streams: the inverse of fqsx_idg_encode_block / fqsx_id_encode_block, and what the reference's
 * `fqs d` writes (CIdCompressor::Decompress / DecompressPE, fqs/id.cpp:182-228, 495-731) -- not necessarily what the encoder
 * was given: a numeric field comes back as store_int(previous value + delta) (fqs/id.h:117-149: leading zeros are lost), in
 * instrument mode only the instrument name and a line feed come back, id_mode none (host decoder only) gives "@\n".
 * streams[w] / lens[w] = worker w's id stream of the block (host memory); n_reads from the container block; paired as in the
 * encoder.  *ids_out = the block's id lines back to back, each including its line feed, in block order; *id_off_out =
 * n_reads + 1 offsets into it.  Both are callee-owned until the next call.  A codec instance encodes or decodes a file, never both.
 * Errors: a worker with reads to decode and a stream shorter than 8 bytes: FQSX_E_ARG; a malformed or truncated stream (a
 * cumulative frequency at or above its model's total, a move-to-front code beyond the list, bytes wanted beyond the stream's
 * end): FQSX_E_DEVICE -- nothing outside a worker's own output is ever written and the call always returns.  GPU decoder only:
 * a line that would pass 1024 bytes, 128 tokens, an instrument name beyond 62 bytes or more than 4096 names per worker:
 * FQSX_E_DEVICE ("staging sizes" in fqsx_last_error(); decode the file with fqsx_id_decode_block, which has no such limits).
 * The GPU decoder cannot size its model tables and its output from its input: it snapshots them before a block and, when one
 * runs out, restores the snapshot, doubles that capacity and runs the block again ("Reading a file back").
 * FQSX_IDG_INIT=<n> in the environment at fqsx_idg_create: the first table capacities (slots, at least 16) and the first
 * per-worker output capacity of the decoder (bytes, at least 64). */
int fqsx_idg_decode_block(fqsx_idg *, const uint8_t *const *streams, const uint64_t *lens, uint32_t n_reads, int paired,
                          const uint8_t **ids_out, const uint64_t **id_off_out);
/* fqsx_idg_decode_block leaving the block in device memory: *d_ids_out = the block's id lines back to back in block order,
 * *d_id_len_out = their n_reads lengths, *id_bytes_out = the bytes of *d_ids_out.  Both buffers are the codec's, valid until
 * its next call; null on error.  Errors, fqsx_idg_error_kind and the run-again behaviour are those of fqsx_idg_decode_block;
 * the call returns with the codec's stream drained. */
int fqsx_idg_decode_block_dev(fqsx_idg *, const uint8_t *const *streams, const uint64_t *lens, uint32_t n_reads, int paired,
                              const uint8_t **d_ids_out, const uint32_t **d_id_len_out, uint64_t *id_bytes_out);
int fqsx_id_decode_block(fqsx_id *, const uint8_t *const *streams, const uint64_t *lens, uint32_t n_reads, int paired,
                         const uint8_t **ids_out, const uint64_t **id_off_out);
/* out[0] = blocks the decoder ran again, out[1] / out[2] / out[3] = growths of the small table, the big table and the decoder's
 * output, out[4] / out[5] = slots per worker of the small and the big table, out[6] = output bytes per worker, out[7] = 0 */
int fqsx_idg_stats(fqsx_idg *, uint64_t out[8]);
/* out[4 * w + 0 / 1 / 2] = models in worker w's small table, in its big table, names in its move-to-front list after the last
 * block (an encoder and a decoder that have seen the same blocks agree on them) */
int fqsx_idg_state(fqsx_idg *, uint32_t *out);
/* What the kernel reported in the last fqsx_idg_encode_block / fqsx_idg_decode_block: 0 nothing, 5 = a line over 1024 bytes, over
 * 128 tokens or an instrument name over 62 bytes, 6 = more than 4096 instrument names in a worker (5 and 6: the file is for
 * fqsx_id_encode_block / fqsx_id_decode_block), 7 = malformed or truncated stream, 3 / 4 = an output / model table that a valid
 * stream could not have filled; the encoder also: 1 = a byte >= 128, 2 = no instrument name */
int fqsx_idg_error_kind(fqsx_idg *);
/* Kernel timing of the id coder, as fqsx_qual_set_profiling / fqsx_qual_kernel_times: out[0] = milliseconds, out[1] = launches */
int fqsx_idg_set_profiling(fqsx_idg *, int enable);
int fqsx_idg_kernel_times(fqsx_idg *, double out[2]);
int fqsx_idg_separator_times(fqsx_idg *, double out[2]);

/* Read order of `fqs e -om s` with the string work on the GPU.  Replaces preprocess_se
 * (fqs/application.cpp:349-412: 256 bins by the first four bases, N->T) plus CSortedFASTQFile::sort_reads on every
 * bin (fqs/io.h:499-528).  The GPU radix-sorts the reads by the comparator's keys and gives every read a dense
 * rank; the host then runs the same libstdc++ std::sort per bin on the ranks, which reproduces the reference's
 * order of reads that compare equal (ids and qualities follow it).  order_out[n_reads] = read indices, bin after
 * bin; bin_start[257] = offsets of the bins inside order_out. */
int fqsx_sort_order(const uint8_t *bases, const uint64_t *read_off, uint32_t n_reads, int device,
                    uint32_t *order_out, uint32_t *bin_start);
/* The same with bounded device memory, the way the reference bounds its host memory (bins on disk, sorted one after the
 * other, fqs/application.cpp:349-412, 1595-1626): the reads are binned by their first four bases on the host, consecutive
 * bins are packed into batches of at most max_batch_bases bases (a bin larger than that is a batch of its own), and every
 * batch is uploaded and sorted separately.  Same order as fqsx_sort_order (= max_batch_bases 0: one batch).
 * n_batches_out (optional): GPU passes made. */
int fqsx_sort_order_batched(const uint8_t *bases, const uint64_t *read_off, uint32_t n_reads, int device, uint64_t max_batch_bases,
                            uint32_t *order_out, uint32_t *bin_start, uint32_t *n_batches_out);

/* Host-side read order inside one bin of `fqs e -om s`: std::sort with the comparator of
 * CSortedFASTQFile::sort_reads (fqs/io.h:499-528) applied to reads idx_in[0..n) (indices into off[]),
 * result in idx_out.  Same libstdc++ algorithm on the same initial order = same order of equal reads. */
int fqsx_sort_bin(const uint8_t *bases, const uint64_t *off, const uint32_t *idx_in, uint32_t n, uint32_t *idx_out);

/* FASTQ text to columns on the GPU (csrc/fqsx_fastq.h): what the reference's readers do byte by byte (CReadsBlock::get_read,
 * fqs/reads_block.h:35-76; CSortedFASTQFile::get_read, fqs/io.h:451-482).  A line ends at 0x0A only (a 0x0D stays in its
 * field), four line feeds make a record, bytes behind the last fourth line feed belong to no record; any field may be empty.
 * One handle parses one chunk of text at a time and owns its device buffers.  max_chunk_bytes: the chunk size the caller
 * intends to use (0: 256 MiB; below 4 GiB), reported back by fqsx_fastq_max_chunk -- cutting a file into chunks is the
 * caller's job: the unconsumed tail of a chunk goes to the front of the next one, and a chunk without a complete record
 * has to be made longer (fqsqueezer_amd/codec.py: parse_fastq).
 * fqsx_fastq_index: uploads text[0 .. n_bytes) (n_bytes below 4 GiB), finds its line feeds and the field lengths.
 *   out[0] records  out[1] bytes consumed (= position of the first byte that belongs to no record)
 *   out[2] / out[3] / out[4] bytes of the id column (id lines with their line feeds, as read_desc_t::id_len counts them) /
 *   of the base column / of the quality column (both without line feeds)  out[5] the longest id line  out[6] 1 if a
 *   record's quality line and base line differ in length  out[7] line feeds in the chunk
 * fqsx_fastq_columns: the columns of the chunk indexed last, into caller buffers of the sizes fqsx_fastq_index reported:
 *   ids[out[2]], bases[out[3]], quals[out[4]], the three offset arrays with records + 1 entries each (qual_off equals
 *   read_off unless out[6]), plus_len[records] = length of every separator line without its line feed.  A null pointer
 *   skips that array.
 * fqsx_fastq_kernel_times (after fqsx_fastq_set_profiling): out[0..6] = milliseconds of the count, tile scan, index, lengths,
 *   record-tile scan, offsets and gather kernels, out[7..13] = their launches. */
typedef struct fqsx_fastq fqsx_fastq;
int fqsx_fastq_create(int device, uint64_t max_chunk_bytes, fqsx_fastq **out);
void fqsx_fastq_destroy(fqsx_fastq *);
uint64_t fqsx_fastq_max_chunk(fqsx_fastq *);
int fqsx_fastq_index(fqsx_fastq *, const uint8_t *text, uint64_t n_bytes, uint64_t out[8]);
int fqsx_fastq_columns(fqsx_fastq *, uint8_t *ids, uint64_t *id_off, uint8_t *bases, uint64_t *read_off, uint8_t *quals,
                       uint64_t *qual_off, uint32_t *plus_len);
int fqsx_fastq_set_profiling(fqsx_fastq *, int enable);
int fqsx_fastq_kernel_times(fqsx_fastq *, double out[14]);

/* BGZF input (csrc/fqsx_inflate.h): gzip cut into members that do not depend on one another, each at most 64 KiB of text as
 * one raw DEFLATE stream with its own CRC-32 and ISIZE, inflated on the GPU -- one wavefront per member -- into the device
 * buffer the parser reads.  Stored, fixed and dynamic blocks, any number per member; what zlib's inflate accepts is accepted.
 * fqsx_bgzf_scan (host only): walks the member headers of buf[0 .. n_bytes): magic 1f 8b 08, FLG = FEXTRA, the `BC` subfield
 *   with BSIZE = member size - 1.  member_off[i] / isize[i]: offset and ISIZE of the i-th whole member, up to max_members.
 *   out[0] members found  out[1] bytes they span (the first byte behind them)  out[2] bytes behind them (an incomplete member,
 *   or members beyond max_members: the caller carries them into its next read)  out[3] 1 if the bytes at out[1] are no BGZF
 *   member header (a gzip member without `BC`, other flags, no gzip at all), as far as they are there to be judged.  The 28-byte
 *   empty member at a file's end is a member like any other.
 * fqsx_bgzf_inflate: member i is members[member_off[i] .. member_off[i + 1]), the last one ends at n_bytes; uploads them,
 *   inflates them and returns their text back to back in text_out (the sum of their ISIZE bytes, below 4 GiB).
 *   info[0] the first damaged member (n_members: none)  info[1] its kind  info[2] bytes of text  info[3] 0.
 *   Kinds: 1 reserved block type  2 stored LEN / NLEN mismatch  3 over-subscribed or incomplete code (or too many codes, no
 *   end-of-block code)  4 invalid symbol  5 distance before the member's start  6 output beyond ISIZE  7 input exhausted
 *   8 ISIZE mismatch (also an ISIZE above 65536)  9 CRC mismatch  10 no BGZF member header.  A damaged member: FQSX_E_DEVICE,
 *   info and fqsx_last_error name its index and kind, text_out is not written.  The kernel reads nothing outside a member's
 *   bytes and writes nothing outside its ISIZE bytes of text, whatever the member holds.
 * fqsx_fastq_index_bgzf: fqsx_fastq_index on a chunk that is `carry` bytes kept from the end of the previous chunk's text in
 *   device memory (its unconsumed partial record, moved to the front on the device) followed by the inflated members;
 *   carry + the members' text stays below 4 GiB.  out as fqsx_fastq_index (out[1] counts from the carried bytes), info as
 *   fqsx_bgzf_inflate.  fqsx_fastq_columns and fqsx_fastq_columns_into work on the chunk as on any other.  After an error
 *   nothing can be carried: the next chunk starts with carry 0.
 * fqsx_fastq_inflate_times (after fqsx_fastq_set_profiling): out[0] milliseconds, out[1] launches of the inflate kernel. */
int fqsx_bgzf_scan(const uint8_t *buf, uint64_t n_bytes, uint32_t max_members, uint64_t *member_off, uint32_t *isize, uint64_t out[4]);
int fqsx_bgzf_inflate(fqsx_fastq *, const uint8_t *members, uint64_t n_bytes, const uint64_t *member_off, uint32_t n_members,
                      uint8_t *text_out, uint64_t info[4]);
int fqsx_fastq_index_bgzf(fqsx_fastq *, const uint8_t *members, uint64_t n_bytes, const uint64_t *member_off, uint32_t n_members,
                          uint64_t carry, uint64_t out[8], uint64_t info[4]);
int fqsx_fastq_inflate_times(fqsx_fastq *, double out[2]);

/* Device-resident columns (csrc/fqsx_cols.h): a store keeps the base column and the quality column of one input file in
 * device memory, chunk by chunk as the parser produces them -- one allocation per chunk that never moves, so the file is
 * never held twice -- and cuts container blocks out of them by read index.  Ids stay host columns unless the store keeps
 * them too (fqsx_cols_keep_ids).
 * fqsx_cols_info: out[0] records  out[1] bases  out[2] / out[3] device bytes the store holds now / held at most so far.
 * fqsx_fastq_columns_into: what fqsx_fastq_columns does for the chunk indexed last, with the base and quality columns appended
 *   to the store instead of copied to the host; ids[out[2]], id_off, read_off (the chunk's, records + 1 entries from 0) and
 *   plus_len come back as there (a null pointer skips the array).  FQSX_E_ARG, the store unchanged: a chunk with a record
 *   whose quality line differs in length from its base line (the store keeps one offset array for both columns).
 * fqsx_cols_gather: the block whose read i is record idx[i] of store a; with b, read 2i is record idx[i] of a and read 2i + 1
 *   record idx[i] of b (mate 1 / mate 2 of a paired file).  idx[n] and h_off[reads + 1], reads = n or 2 n, are host arrays;
 *   h_off holds the block's offsets (from 0), which the caller knows from the read lengths.  *d_bases, *d_quals and *d_off
 *   (h_off in device memory) are device buffers of store a with h_off[reads] + 64 bytes, valid until the next gather on it;
 *   the call returns with its stream drained.  Every record is checked on the device before anything is stored: an index
 *   that is no record of the store, or offsets that give a read another length than the store holds: FQSX_E_ARG; a range
 *   outside a buffer: FQSX_E_DEVICE.  A refused call leaves the buffers of the previous block as they were.
 * fqsx_cols_bases: the whole base column into out[bases].
 * fqsx_cols_sort_order: the read order of `fqs e -om s` for the records of the store, computed where they lie: the same
 *   order_out / bin_start as fqsx_sort_order on the same reads.  No read is copied: the sort reads every record through its
 *   device address, and what it allocates on the store (per record 8 address + 4 length + 1 bin + 8 permutations + 4 flags +
 *   4 rank bytes, about 0.5 more for the tiles, 72 per chunk) is handed back before it returns -- also when an allocation
 *   fails (FQSX_E_NOMEM; the call can be repeated).  Only the ranks and the bins come to the host, which replays std::sort
 *   per bin as fqsx_sort_order does.  An empty store: bin_start all zero.  info_out (optional): [0] radix passes [1] scratch
 *   bytes allocated at most during the call [2] records [3] 0.  A record outside its chunk: FQSX_E_DEVICE, order_out unwritten.
 * fqsx_cols_download: n_bytes of the store's device memory (a gathered block) to the host.
 * fqsx_cols_kernel_times (after fqsx_cols_set_profiling): out[0] / out[1] milliseconds and launches of the copying gather,
 *   out[2] / out[3] of the checking pass in front of it.
 * fqsx_cols_keep_ids: before the first chunk is appended, makes the store keep the id column beside the two others; afterwards
 *   FQSX_E_ARG, the store unchanged.  On such a store fqsx_fastq_columns_into gives the chunk's one allocation two more parts,
 *   each 16-byte aligned -- the chunk's own id_off (records + 1 entries from 0) and its id lines with their line feeds -- and
 *   the parser writes the lines there; `ids` may then be null, and no id byte comes to the host.  id_off, read_off and plus_len
 *   come back as before.
 * fqsx_cols_gather_ids: fqsx_cols_gather for the id column, with the same index semantics (with b the mates' lines interleaved),
 *   the same check-then-store passes, error texts and return codes.  h_id_off[reads + 1]: the block's id offsets (from 0), which
 *   the caller knows from the line lengths.  *d_ids (h_id_off[reads] + 64 bytes) and *d_id_off are buffers of store a of their
 *   own, not the ones of fqsx_cols_gather: a block's bases and its ids are valid at the same time, each until the next gather of
 *   its kind.  A refused call leaves the previous block's ids and offsets as they were.  The call returns with the stream
 *   drained.  FQSX_E_ARG if a, or a given b, does not keep ids.
 * fqsx_cols_id_info: out[0] 1 if the store keeps ids  out[1] the id bytes it holds.
 * fqsx_cols_id_survey: one kernel over the id lines of all records, for the id kernel's staging limits (fqsx_idg_*):
 *   out[0] 1 if the store keeps ids  out[1] the id bytes held  out[2] the longest id line, with its line feed  out[3] the most
 *   tokens in a line (bytes outside [0-9A-Za-z@], the line feed included)  out[4] the longest instrument name among the lines
 *   that have one (up to the first of '.', ' ', ':', cut short at a NUL)  out[5] the most tokens up to the name's end plus its
 *   terminator among those lines  out[6], out[7] 0.  A store without ids or without records: all zero apart from out[0].  A
 *   record outside its chunk or a line outside its chunk's ids: FQSX_E_DEVICE.
 * fqsx_cols_id_kernel_times (after fqsx_cols_set_profiling): milliseconds and launches of the id gather's checking pass
 *   (out[0], out[1]), of its copying pass (out[2], out[3]) and of the survey (out[4], out[5]). */
typedef struct fqsx_cols fqsx_cols;
int fqsx_cols_create(int device, fqsx_cols **out);
void fqsx_cols_destroy(fqsx_cols *);
int fqsx_cols_info(fqsx_cols *, uint64_t out[4]);
int fqsx_fastq_columns_into(fqsx_fastq *, fqsx_cols *, uint8_t *ids, uint64_t *id_off, uint64_t *read_off, uint32_t *plus_len);
int fqsx_cols_gather(fqsx_cols *a, fqsx_cols *b, const uint32_t *idx, uint32_t n, const uint64_t *h_off, const uint8_t **d_bases,
                     const uint8_t **d_quals, const uint64_t **d_off);
int fqsx_cols_bases(fqsx_cols *, uint8_t *out);
int fqsx_cols_sort_order(fqsx_cols *, uint32_t *order_out, uint32_t *bin_start /*[257]*/, uint64_t info_out[4]);
int fqsx_cols_download(fqsx_cols *, const void *d_src, void *h_dst, uint64_t n_bytes);
int fqsx_cols_set_profiling(fqsx_cols *, int enable);
int fqsx_cols_kernel_times(fqsx_cols *, double out[4]);
int fqsx_cols_keep_ids(fqsx_cols *);
int fqsx_cols_gather_ids(fqsx_cols *a, fqsx_cols *b, const uint32_t *idx, uint32_t n, const uint64_t *h_id_off, const uint8_t **d_ids,
                         const uint64_t **d_id_off);
int fqsx_cols_id_info(fqsx_cols *, uint64_t out[2]);
int fqsx_cols_id_survey(fqsx_cols *, uint64_t out[8]);
int fqsx_cols_id_kernel_times(fqsx_cols *, double out[6]);

/* Columns to FASTQ text on the device (csrc/fqsx_fqtext.h): the text `fqs d` writes for one container block, from the columns
 * the *_decode_block_dev entry points leave in device memory.  Per read: id line (with its line feed) + bases + "\n+\n" +
 * qualities + "\n"; paired != 0: read i goes to output i & 1 (application.cpp:871-889, 980-982).
 * fqsx_fqtext_block: ids = the id lines back to back (id_bytes of them) and id_len[n_reads] their lengths, both in device
 *   memory (ids_on_device != 0) or both host arrays that the call uploads; ids == NULL: every id line is "@\n".  d_bases /
 *   d_quals: device columns under h_read_off (host, n_reads + 1 offsets from 0); d_quals == NULL: every quality is the byte
 *   qual_fill.  text_bytes[m] = bytes of output m.  The call reads buffers other handles own -- their streams must be
 *   drained -- and returns when the text is complete in the handle's own buffers.  Every record is checked on the device
 *   before anything is stored: offsets that do not ascend, a read of 2^24 bases or more, an id line of 0 bytes, id lengths
 *   that do not add up to id_bytes, paired with an odd n_reads: FQSX_E_ARG; a range outside a buffer: FQSX_E_DEVICE.  A
 *   refused call leaves the text of the previous block as it was.
 * fqsx_fqtext_download: output `mate` of the block assembled last into dst[text_bytes[mate]] (through a pinned staging buffer).
 *   Calls on one handle are serialised by the caller: a download may run on another host thread while the decoders work on
 *   the next block, but the next fqsx_fqtext_block waits for it.
 * fqsx_fqtext_kernel_times (after fqsx_fqtext_set_profiling): out[0..3] = milliseconds of the size, tile scan, offset and
 *   scatter kernels, out[4..7] = their launches. */
typedef struct fqsx_fqtext fqsx_fqtext;
int fqsx_fqtext_create(int device, fqsx_fqtext **out);
void fqsx_fqtext_destroy(fqsx_fqtext *);
int fqsx_fqtext_block(fqsx_fqtext *, uint32_t n_reads, int paired, const uint8_t *ids, const uint32_t *id_len, int ids_on_device,
                      uint64_t id_bytes, const uint8_t *d_bases, const uint8_t *d_quals, int qual_fill, const uint64_t *h_read_off,
                      uint64_t text_bytes[2]);
int fqsx_fqtext_download(fqsx_fqtext *, int mate, uint8_t *dst);
int fqsx_fqtext_set_profiling(fqsx_fqtext *, int enable);
int fqsx_fqtext_kernel_times(fqsx_fqtext *, double out[8]);

const char *fqsx_last_error(void);
const char *fqsx_version(void);

#ifdef __cplusplus
}
#endif
#endif
