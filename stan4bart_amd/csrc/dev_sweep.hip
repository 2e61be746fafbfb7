// Translation unit of the persistent tree sweep (k_sweep*, k_sbatch*): the shared device headers, the interface the host driver sees
// (dev_sweep_api.hpp) and the kernels (dev_sweep.inc).  A unit of its own because it is compiled with -mllvm -disable-machine-licm
// (Makefile): the kernel is one long loop over the trees, and hoisting every loop-invariant constant and mask out of it costs ~190
// more spilled vector registers than it saves instructions.
#include <hip/hip_runtime.h>
// Measurement macros of this unit that tree_hd.hpp expands (the SW_* timers are in dev_sweep.inc); empty unless defined here.
#ifdef S4B_SWEEP_TIMING
// (measurement build `make sweeptiming`) time stamps inside decide() of the decider wave of workgroup 100 of k_sweep: sums of absolute clock
// values per slot ([15] = calls), read back by sweep_decide_fetch and printed as differences by profile_sweep_persistent (dev_hip.hip)
__device__ unsigned long long g_dec[16];
// ([i] = sum of (now - entry) over the calls that reach stamp i, [8 + i] = how many did; [0] holds the entry time of the call in flight)
#define S4B_DEC_T(i) do { if (blockIdx.x == 100 && threadIdx.x == 0) { if ((i) == 0) { g_dec[0] = (unsigned long long)wall_clock64(); atomicAdd(&g_dec[15], 1ull); } \
                                                                      else { atomicAdd(&g_dec[i], (unsigned long long)wall_clock64() - g_dec[0]); atomicAdd(&g_dec[7 + (i)], 1ull); } } } while (0)
#endif
#include "dev_wave.hpp"
#include "dev_control.hpp"
#include "dev_step_shared.hpp"
#include "dev_sweep_api.hpp"
#include "dev_sweep.inc"
