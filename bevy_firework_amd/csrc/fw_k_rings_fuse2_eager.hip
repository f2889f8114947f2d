// fw_k_rings_fuse2_eager.hip -- the fused forms of the FIFO ring kernel whose spawning workgroups spin what they spawn, the eager rule of
// rounds 19 to 26 (fw_k_update_fifo2_eager; round 27, fw_spin.h: fw_spin_newborn_deferred): the lines of fw_k_rings_fuse2.hip, in a unit
// of their own so that the two sets of 28 kernels compile side by side.  Launched where FwFifoArgs::fuse_pad[FW_FIFO_NEWBORN] is 0:
// FW_NEWBORN_SPIN=1.
#define FW_FUSE2_EAGER
#include "fw_k_rings_fuse2.hip"
