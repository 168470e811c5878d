// fqsx_insplan.h -- the draw rule of the window-parallel insert phase (fqsx_dev.h: insert_windows), as pure functions
// that compile for the device and for the host alike: the kernel and the CPU model of tests/test_insert_plan.py
// read the same text.
//
// A window is a stretch of an owner's key group that is applied at once.  For one occurrence of a k-mer in it:
//   c0  the k-mer's counter before the window (0: not in the table)
//   r   the number of earlier occurrences of the same k-mer in the window (its rank)
// Increments at counts <= thr are certain and a counter never decreases, so the counter this occurrence meets is
// exactly c0 + r while c0 + r <= thr, and certainly > thr otherwise -- whatever the draws of the earlier occurrences
// gave.  Whether it takes a number from the owner's MT19937 stream (the in-order rule: thr < counter < maxv) is
// therefore known before any draw is made, except when the earlier occurrences may or may not have carried the
// counter up to maxv.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) && !defined(FQSX_EMU)
#define FQ_PLAN __host__ __device__ inline
#else
#define FQ_PLAN inline
#endif

// the occurrence takes the next number of the stream
FQ_PLAN bool insplan_draws(uint32_t c0, uint32_t r, uint32_t thr, uint32_t maxv) { return c0 + r > thr && c0 + r < maxv; }
// ... or nobody can say without the earlier draws: the counter was below maxv and may have reached it by now
// (the whole window is then applied in order)
FQ_PLAN bool insplan_ambiguous(uint32_t c0, uint32_t r, uint32_t thr, uint32_t maxv) {
  (void)thr;
  return c0 < maxv && c0 + r >= maxv;
}
// the step of an occurrence that meets counter value cnt (> 0: the key is in the table): does it add one?
// draws / rnd: insplan_draws of the occurrence and the number it took; cm: the largest value the field holds
FQ_PLAN bool insplan_adds(uint32_t cnt, bool draws, uint32_t rnd, uint32_t thr, uint32_t mult, uint32_t cm) {
  if (cnt <= thr) return cnt < cm;
  return draws && rnd % (mult * (cnt - thr)) == 0;
}
