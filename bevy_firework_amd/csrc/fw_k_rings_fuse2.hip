// fw_k_rings_fuse2.hip -- the FIFO ring kernel's form that runs TWO frames of a spin-less launch in one pass (FwFifoArgs::fused, fw_fuse2.h,
// DESIGN.md 4.0, round 22): fw_k_update_fifo2, the FUSE2 arm of fw_update_fifo_body, instantiated here and nowhere else.  A unit of its
// own so that fw_k_rings.hip compiles to what it compiled to before the form existed: the templates come from there.
#define FW_RINGS_TEMPLATES_ONLY
#include "fw_k_rings.hip"

hipError_t fw_launch_update_fifo2(hipStream_t s, const FwGlobals &g, const FwFifoArgs &a, const FwInlineOps &inl, uint32_t total_tiles, int nt,
                                  hipEvent_t e0, hipEvent_t e1) {
    if (!total_tiles || !a.n_segs || !a.fused || !a.spinless || !a.q0pl || a.any_inst || a.small_tiles) return hipErrorInvalidValue;
    const dim3 grid(total_tiles), block(FW_BLOCK);
    // (the forms of the spin-less launch: fully and write-only non-temporal, write mask 0 and generic)
    if (nt == 2)
        FW_LAUNCH_T((fw_k_update_fifo2<-1, 2>), grid, block, s, e0, e1, g, a, inl);
    else if (nt)
        FW_LAUNCH_T((fw_k_update_fifo2<-1, 1>), grid, block, s, e0, e1, g, a, inl);
    else if (a.write_mask == 0)
        FW_LAUNCH_T((fw_k_update_fifo2<0, 0>), grid, block, s, e0, e1, g, a, inl);
    else
        FW_LAUNCH_T((fw_k_update_fifo2<-1, 0>), grid, block, s, e0, e1, g, a, inl);
    return hipGetLastError();
}
