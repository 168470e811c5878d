// fqsx_split.h -- how a reads block is split among the T workers and into synchronisation segments: the format's rule, in
// one place for the kernels, the host orchestration (fqsx_api.hip) and the host coders (fqsx_host.cpp, plain g++).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) && !defined(FQSX_EMU)
#define FQSX_SPLIT_FN __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))   /* (no HIP header needed) */
#else
#define FQSX_SPLIT_FN static inline
#endif

// PartitionForWorkers, reads_block.h:197-214: worker t of T codes reads [first, last) of the block's n_reads; the inner
// boundaries are even, so that the mates of a pair stay with one worker
FQSX_SPLIT_FN void worker_reads(uint64_t t, uint64_t T, uint64_t n_reads, uint64_t &first, uint64_t &last) {
  first = t * n_reads / T;
  last = (t + 1) * n_reads / T;
  if (t) first &= ~1ull;
  if (t + 1 < T) last &= ~1ull;
}

// next_synchro of segment seg < S (application.cpp:643): a worker with reads [first, last) synchronises after the read with
// this index (single-end), after the first pair that reaches it (paired-end, application.cpp:1170)
FQSX_SPLIT_FN uint64_t segment_synchro(uint64_t seg, uint64_t S, uint64_t first, uint64_t last) {
  return (seg + 1) * (last - first) / (S + 1) + first;
}
