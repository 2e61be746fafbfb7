// Batched launches of the solo sweep (k_sbatch*, dev_sweep.inc; launched by the sweep group of dev_hip.hip).  Workgroup b of such a launch
// runs member b's sweep exactly as a one-workgroup launch of that member would: its arguments sit in slot b of a device buffer, laid out as
// the kernarg segment is (BartArrays, then SweepArgs), and every use of the launch geometry in sweep_body goes through the logical pair
// SW_BX / SW_GX — workgroup 0 of a grid of 1 under BATCH, a template constant of the function that expands them.  With BATCH false both are
// the hardware values and the kernels of one sampler compile to the code they always had.
#define SW_BX (BATCH ? 0u : blockIdx.x)
#define SW_GX (BATCH ? 1u : gridDim.x)
// (BATCH: the one kernel argument is the address of the slots; the member's arguments are read from its slot through the same constant
// address space as the kernarg segment, so every argument load stays a scalar load)
typedef const __attribute__((address_space(4))) unsigned char* sw_karg_ptr;
__device__ __forceinline__ sw_karg_ptr sw_batch_slot(sw_karg_ptr kp) {
  return (sw_karg_ptr)(*(const __attribute__((address_space(4))) unsigned long long*)kp + (unsigned long long)blockIdx.x * SW_SLOT_BYTES);
}
#define SW_SLOT_OF(kp) if constexpr (BATCH) kp = sw_batch_slot(kp)      // (no do-while: a loop scope would renumber the cleanup destinations of every kernel)
