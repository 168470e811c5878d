// fqsx_k_code.hip -- deferred coding (single-end sorted blocks, the phases that are followed by another phase): the encode
// kernel that leaves its coding to a later launch, and the kernel that does it.  A translation unit of its own, so that the
// unit of the kernels that code themselves (fqsx_k_se.hip) compiles to the code object it compiled to without these.
#include "fqsx_roles.h"

#ifndef FQSX_EMU
// The eight-wave workgroup of k_encode_se_sorted without its coding: the resolving wave leaves the phase's queue entries in
// device memory (DevCfg.gq[a.defer - 1], tagged a.seq) and touches no coder state; waves 3 and 4 have nothing to do.
FQ_KERNEL512 void k_encode_se_sorted_defer(EncArgs a) {
  if (wg_handoff_init(a, true)) return;   // the block's queue has been stopped (fqsx_api.hip: phase_skip)
  switch (FQ_WAVE_ID) {
    case 0: role_head(fq_kernarg()); break;
    case 1: role_scout(fq_kernarg(), 0u); break;
    case 2: role_resolve<1, true>(fq_kernarg()); break;
    case 3: case 4: break;
    case 5: role_inserter(fq_kernarg()); break;
    case 6: role_scout(fq_kernarg(), 2u); break;
    default: role_scout(fq_kernarg(), 1u); break;
  }
}
// The models and the range coder of such a phase, over the queue its encode launch (a.seq) left in device memory.  Three
// waves per worker: feeder, models, range coder.  Runs on the codec's second stream beside the phase's partition and insert
// kernels and the next phase's encode launch, none of which reads or writes what it does: the worker's context models,
// averages, coder state and output stream.  A growth posted meanwhile (err[1]) does not stop it -- the phase's symbols
// are due either way.  (The workgroup holds the whole WgShared although it uses the two queue rings and the models' scratch
// only: it takes a compute unit to itself, see DESIGN.md.)
FQ_KERNEL512 void k_code_se_sorted(EncArgs a) {
  const GQueue &q = a.cfg.gq[a.defer - 1];
  if (wg_handoff_init(a, false, q.tag[FQ_BLOCK] != a.seq)) return;
  switch (FQ_WAVE_ID) {
    case 0: role_feeder(fq_kernarg()); break;
    case 1: role_models(fq_kernarg()); break;
    default: role_rc(fq_kernarg()); break;
  }
}
int fqsx_launch_encode_se_defer(hipStream_t s, const EncArgs &a) {
  hipLaunchKernelGGL(k_encode_se_sorted_defer, dim3(a.cfg.T), dim3(512), 0, s, a);
  return (int)hipGetLastError();
}
int fqsx_launch_code_se(hipStream_t s, const EncArgs &a) {
  hipLaunchKernelGGL(k_code_se_sorted, dim3(a.cfg.T), dim3(3 * 64), 0, s, a);
  return (int)hipGetLastError();
}
#endif
