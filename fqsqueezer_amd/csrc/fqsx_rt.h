// fqsx_rt.h -- the device context of a codec and the runtime steps on it.
//
// Every codec of fqsx_api.hip (fqsx_dna, fqsx_qual, fqsx_idg, the sort) is a DevCtx: one device, one stream, the two timing
// events, the kernel-time counters and the ledger of its allocations.  The steps below are the only place that talks to
// the HIP runtime on the codec's behalf; the FQSX_EMU build implements the same steps with host memory and runs a kernel
// as a loop over its blocks, so that the host orchestration is one piece of code in both builds.
#pragma once
#include "fqsx_plat.h"
#include "../../include/fqsx.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static thread_local std::string g_err;

#ifndef FQSX_EMU
typedef hipStream_t DevStream;
typedef hipEvent_t DevEvent;
#else
typedef void *DevStream;   // (the emulation has neither: everything runs on the calling thread)
typedef void *DevEvent;
#endif

struct DevCtx {
  int device = 0;
  DevStream stream = nullptr;
  DevEvent ev0 = nullptr, ev1 = nullptr;   // around every launch while profiling
  bool profiling = false;
  // a second stream for work that only has to be finished at a join (dev_side_open; the DNA encoder's deferred coding):
  // launch k (0 / 1, the two buffers it alternates between) starts behind ev_fork[k], recorded on the first stream, and ends at ev_done[k]
  DevStream side = nullptr;
  DevEvent ev_fork[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr};   // (timing disabled)
  bool side_used[2] = {false, false};   // ev_done[k] has been recorded and not yet been seen complete / waited for
  int side_last = -1;                   // the k of the side stream's last launch while the first stream has not joined it
  double k_ms[3] = {0, 0, 0};   // kernel time per index: 0 encode / decode (the quality and id kernels), 1 insert phase, 2 the rest
  u64 k_n[3] = {0, 0, 0};       // ... and launches timed (the emulation build and fqsx_dna's index 0: every launch)
  std::vector<void *> allocs;
  std::vector<u64> alloc_bytes;   // size of allocs[i]
  u64 dev_bytes = 0, dev_bytes_peak = 0;   // device memory held now / at most so far (fqsx_dna_capacity)
  u64 n_dalloc = 0;   // dalloc calls so far (FQSX_TEST_ALLOC_FAIL)
};

#ifndef FQSX_EMU
#define HIPCHK(x)                                                                             \
  do {                                                                                        \
    hipError_t e_ = (x);                                                                      \
    if (e_ != hipSuccess) {                                                                   \
      g_err = std::string(#x) + ": " + hipGetErrorString(e_);                                 \
      return FQSX_E_HIP;                                                                      \
    }                                                                                         \
  } while (0)

// device checks, the device made current, the stream -- with n_parts > 1 one whose kernels only run on compute-unit
// partition `part` of n_parts -- and the timing events
static int dev_open(DevCtx *c, int device, u32 part = 0, u32 n_parts = 1) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    g_err = "no HIP device available (libfqsx has no CPU path)";
    return FQSX_E_NO_DEVICE;
  }
  if (device < 0 || device >= ndev) { g_err = "bad device ordinal"; return FQSX_E_ARG; }
  HIPCHK(hipSetDevice(device));
  c->device = device;
  hipError_t se;
  if (n_parts > 1) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) { g_err = "hipGetDeviceProperties failed"; return FQSX_E_HIP; }
    const u32 ncu = (u32)prop.multiProcessorCount, lo = (u32)((u64)part * ncu / n_parts), hi = (u32)(((u64)part + 1) * ncu / n_parts);
    std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
    for (u32 i = lo; i < hi; ++i) mask[i / 32] |= 1u << (i % 32);
    se = hipExtStreamCreateWithCUMask(&c->stream, (uint32_t)mask.size(), mask.data());
  } else
    se = hipStreamCreate(&c->stream);
  if (se != hipSuccess || hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) {
    g_err = "hipStreamCreate / hipEventCreate failed";
    return FQSX_E_HIP;
  }
  return FQSX_OK;
}
static int dev_enter(DevCtx *c) {
  HIPCHK(hipSetDevice(c->device));
  return FQSX_OK;
}
static int dev_sync(DevCtx *c) {
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->side_last >= 0) {   // (work the first stream has not joined: the host waits for both)
    HIPCHK(hipStreamSynchronize(c->side));
    c->side_used[0] = c->side_used[1] = false;
    c->side_last = -1;
  }
  return FQSX_OK;
}
// ---- the second stream
static int dev_side_open(DevCtx *c) {
  if (c->side) return FQSX_OK;
  HIPCHK(hipStreamCreate(&c->side));
  for (int k = 0; k < 2; ++k) {
    HIPCHK(hipEventCreateWithFlags(&c->ev_fork[k], hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_done[k], hipEventDisableTiming));
  }
  return FQSX_OK;
}
// `launch` (which returns its hipError_t) on the second stream, behind everything the first stream holds so far
template <class F> static int dev_side_launch(DevCtx *c, u32 k, F &&launch) {
  HIPCHK(hipEventRecord(c->ev_fork[k], c->stream));
  HIPCHK(hipStreamWaitEvent(c->side, c->ev_fork[k], 0));
  const int e = launch();
  if (e) { g_err = std::string("kernel launch: ") + hipGetErrorString((hipError_t)e); return FQSX_E_HIP; }
  HIPCHK(hipEventRecord(c->ev_done[k], c->side));
  c->side_used[k] = true;
  c->side_last = (int)k;
  return FQSX_OK;
}
// What the first stream launches next comes behind side launch k.  The event is asked first: it is mostly complete, and
// then the stream is spared the wait.
static int dev_side_wait(DevCtx *c, u32 k) {
  if (!c->side_used[k]) return FQSX_OK;
  const hipError_t q = hipEventQuery(c->ev_done[k]);
  if (q == hipErrorNotReady) {
    (void)hipGetLastError();   // ("not ready" is an answer, not a failure to be found by the next launch check)
    HIPCHK(hipStreamWaitEvent(c->stream, c->ev_done[k], 0));
  } else
    HIPCHK(q);
  c->side_used[k] = false;
  return FQSX_OK;
}
// ... behind everything the second stream holds (its launches end in order)
static int dev_side_join(DevCtx *c) {
  if (c->side_last < 0) return FQSX_OK;
  const int rc = dev_side_wait(c, (u32)c->side_last);
  if (rc) return rc;
  c->side_used[0] = c->side_used[1] = false;
  c->side_last = -1;
  return FQSX_OK;
}
// the second stream drained and handed back with its events (dev_side_open makes a new one when it is wanted again)
static void dev_side_close(DevCtx *c) {
  if (!c->side) return;
  (void)hipStreamSynchronize(c->side);
  for (int k = 0; k < 2; ++k) {
    if (c->ev_fork[k]) (void)hipEventDestroy(c->ev_fork[k]);
    if (c->ev_done[k]) (void)hipEventDestroy(c->ev_done[k]);
    c->ev_fork[k] = c->ev_done[k] = nullptr;
    c->side_used[k] = false;
  }
  (void)hipStreamDestroy(c->side);
  c->side = nullptr;
  c->side_last = -1;
}
static int dev_malloc(void **p, u64 bytes) {
  const hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) {
    g_err = "hipMalloc(" + std::to_string(bytes) + "): " + hipGetErrorString(e);
    return FQSX_E_NOMEM;
  }
  return FQSX_OK;
}
static void dev_free_raw(void *p) { (void)hipFree(p); }
static int dfill(DevCtx *c, void *p, int byte, u64 bytes) {
  HIPCHK(hipMemsetAsync(p, byte, bytes, c->stream));
  return FQSX_OK;
}
static int h2d(DevCtx *c, void *d, const void *h, u64 bytes) {
  HIPCHK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
  return FQSX_OK;
}
static int d2d(DevCtx *c, void *d, const void *s, u64 bytes) {
  HIPCHK(hipMemcpyAsync(d, s, bytes, hipMemcpyDeviceToDevice, c->stream));
  return FQSX_OK;
}
// (asynchronous: h is written once the stream gets there)
static int d2h(DevCtx *c, void *h, const void *d, u64 bytes) {
  HIPCHK(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream));
  return FQSX_OK;
}
static int pinned_alloc(void **p, u64 bytes) {
  HIPCHK(hipHostMalloc(p, bytes));
  return FQSX_OK;
}
static void pinned_free(void *p) {
  if (p) (void)hipHostFree(p);
}
// (teardown: errors are not reported)
static void dev_drain(DevCtx *c) {
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  if (c->side) (void)hipStreamSynchronize(c->side);
  c->side_used[0] = c->side_used[1] = false;
  c->side_last = -1;
}
static void dev_destroy_stream(DevCtx *c) {
  (void)hipEventDestroy(c->ev0);
  (void)hipEventDestroy(c->ev1);
  (void)hipStreamDestroy(c->stream);
  dev_side_close(c);
}
// One launch on the context's stream (`launch` returns its hipError_t).  While profiling it is timed between the two
// events, waited for, and counted; `count`: counted in any case.
template <class F> static int dev_launch(DevCtx *c, u32 kidx, bool count, F &&launch) {
  if (c->profiling) HIPCHK(hipEventRecord(c->ev0, c->stream));
  const int e = launch();
  if (e) { g_err = std::string("kernel launch: ") + hipGetErrorString((hipError_t)e); return FQSX_E_HIP; }
  if (c->profiling) {
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    HIPCHK(hipEventSynchronize(c->ev1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->k_ms[kidx] += ms;
  }
  if (c->profiling || count) c->k_n[kidx] += 1;
  return FQSX_OK;
}
// (the body of LAUNCH's launch function)
#define DEV_KERNEL(c, kern, grid, block, ...)                                  \
  hipLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, (c)->stream, __VA_ARGS__); \
  return (int)hipGetLastError()
#else  // ---------------------------------------------------------------- host emulation
static int dev_open(DevCtx *c, int device, u32 = 0, u32 = 1) {
  c->device = device;
  return FQSX_OK;
}
static int dev_enter(DevCtx *) { return FQSX_OK; }
static int dev_sync(DevCtx *) { return FQSX_OK; }
static int dev_side_join(DevCtx *) { return FQSX_OK; }   // (there is no second stream)
static int dev_malloc(void **p, u64 bytes) {
  *p = malloc(bytes);
  if (!*p) { g_err = "host allocation failed"; return FQSX_E_NOMEM; }
  return FQSX_OK;
}
static void dev_free_raw(void *p) { free(p); }
static int dfill(DevCtx *, void *p, int byte, u64 bytes) {
  memset(p, byte, bytes);
  return FQSX_OK;
}
static int h2d(DevCtx *, void *d, const void *h, u64 bytes) {
  memcpy(d, h, bytes);
  return FQSX_OK;
}
static int d2d(DevCtx *, void *d, const void *s, u64 bytes) {
  memcpy(d, s, bytes);
  return FQSX_OK;
}
static int d2h(DevCtx *, void *h, const void *d, u64 bytes) {
  memcpy(h, d, bytes);
  return FQSX_OK;
}
static int pinned_alloc(void **p, u64 bytes) { return dev_malloc(p, bytes); }
static void pinned_free(void *p) { free(p); }
static void dev_drain(DevCtx *) {}
static void dev_destroy_stream(DevCtx *) {}
template <class F> static int dev_launch(DevCtx *c, u32 kidx, bool, F &&launch) {
  launch();
  c->k_n[kidx] += 1;
  return FQSX_OK;
}
// the kernel's blocks one after the other on this thread
template <class F> static int emu_grid(u32 grid, F &&block) {
  fq_emu_nblocks = grid;
  for (u32 b = 0; b < grid; ++b) {
    fq_emu_block = b;
    block();
  }
  return 0;
}
#define DEV_KERNEL(c, kern, grid, block, ...) return emu_grid((u32)(grid), [&] { kern(__VA_ARGS__); })
#endif

// returns from the caller with the code of a step that failed
#define DEVCHK(x)                 \
  do {                            \
    const int rc_ = (x);          \
    if (rc_) return rc_;          \
  } while (0)
// kernel `kern` over `grid` workgroups of `block` threads, timed under kernel index kidx (returns from the caller on failure)
#define LAUNCH(c, kidx, kern, grid, block, ...) \
  DEVCHK(dev_launch(c, kidx, false, [&] { DEV_KERNEL(c, kern, grid, block, __VA_ARGS__); }))

// ---- allocations: every one is in the context's ledger, so that dev_close can hand back whatever is left
static int dzero(DevCtx *c, void *p, u64 bytes) { return dfill(c, p, 0, bytes); }
static int dfill_ff(DevCtx *c, void *p, u64 bytes) { return dfill(c, p, 0xff, bytes); }
// (tests: FQSX_TEST_ALLOC_FAIL=k makes the context's k-th dalloc, counted from 0, fail before it touches the runtime)
static int dalloc(DevCtx *c, void **p, u64 bytes, bool zero) {
  if (bytes == 0) bytes = 8;
  const char *fail_at = getenv("FQSX_TEST_ALLOC_FAIL");
  if (c->n_dalloc++ == (fail_at ? strtoull(fail_at, nullptr, 10) : ~0ull)) {
    g_err = "allocation " + std::string(fail_at) + " of the context refused (FQSX_TEST_ALLOC_FAIL)";
    return FQSX_E_NOMEM;
  }
  int rc = dev_malloc(p, bytes);
  if (rc) return rc;
  if (zero && (rc = dzero(c, *p, bytes))) { dev_free_raw(*p); return rc; }
  c->allocs.push_back(*p);
  c->alloc_bytes.push_back(bytes);
  c->dev_bytes += bytes;
  c->dev_bytes_peak = std::max(c->dev_bytes_peak, c->dev_bytes);
  return FQSX_OK;
}
static void dfree(DevCtx *c, void *p) {
  if (!p) return;
  auto it = std::find(c->allocs.begin(), c->allocs.end(), p);
  if (it != c->allocs.end()) {
    const size_t i = it - c->allocs.begin();
    c->dev_bytes -= c->alloc_bytes[i];
    c->alloc_bytes.erase(c->alloc_bytes.begin() + i);
    c->allocs.erase(it);
  }
  dev_free_raw(p);
}
static void dfree_all(DevCtx *c) {
  const std::vector<void *> a = c->allocs;
  for (void *p : a) dfree(c, p);
}
// The one way a buffer that is reused from call to call grows: nothing if `need` units fit into `cap`; else the old buffer is
// handed back and FORGOTTEN (ptr null, cap 0) before its successor of `new_cap` units of `unit_bytes` bytes is asked for, so
// that a failed allocation leaves nothing dangling and the next call starts from an empty buffer.  new_cap: the site's own rule.
template <class P, class C> static int dfit(DevCtx *c, P *&ptr, C &cap, u64 need, u64 new_cap, u64 unit_bytes, bool zero = false) {
  if (need <= cap) return FQSX_OK;
  dfree(c, (void *)ptr);
  ptr = nullptr;
  cap = 0;
  void *p = nullptr;
  const int rc = dalloc(c, &p, new_cap * unit_bytes, zero);
  if (rc) return rc;
  ptr = (P *)p;
  cap = (C)new_cap;
  return FQSX_OK;
}
static int d2h_sync(DevCtx *c, void *h, const void *d, u64 bytes) {
  int rc = d2h(c, h, d, bytes);
  return rc ? rc : dev_sync(c);
}
// the device made current, the stream drained, every allocation handed back, the stream and the events destroyed
static void dev_close(DevCtx *c) {
  dev_drain(c);
  dfree_all(c);
  dev_destroy_stream(c);
}
