// fw_k_rings_fuse2.hip -- the FIFO ring kernel's forms that run SEVERAL frames of a spin-less launch in one pass (FwFifoArgs::fused = the
// depth, FwFuseArgs, fw_fuse2.h, DESIGN.md 4.0, rounds 22 to 24): fw_k_update_fifo2<D, WM, NT>, the FUSE arm of fw_update_fifo_body,
// instantiated here and nowhere else -- depths 2 to 8 over the four forms of the spin-less launch.  A unit of its own so that
// fw_k_rings.hip compiles to what it compiled to before the forms existed: the templates come from there.
// One instantiation per depth, never a run-time depth: with the loops over FwFuseArgs left rolled the compiler indexes the by-value
// argument record dynamically and copies it to private memory -- 141 VGPRs, 1928 B of scratch per lane, three waves (round 24).  Every
// depth is launched: the default groups close at fw_ctx::fuse_depth, and a reader may flush a group of any depth from 2 to 7.
#define FW_RINGS_TEMPLATES_ONLY
#include "fw_k_rings.hip"

// (the forms of the spin-less launch: fully and write-only non-temporal, write mask 0 and generic)
template <int D>
static hipError_t fw_launch_fifo2_depth(hipStream_t s, const FwGlobals &g, const FwFifoArgs &a, const FwInlineOps &inl, const FwFuseArgs &fz, dim3 grid,
                                        dim3 block, int nt, hipEvent_t e0, hipEvent_t e1) {
    if (nt == 2)
        FW_LAUNCH_T((fw_k_update_fifo2<D, -1, 2>), grid, block, s, e0, e1, g, a, inl, fz);
    else if (nt)
        FW_LAUNCH_T((fw_k_update_fifo2<D, -1, 1>), grid, block, s, e0, e1, g, a, inl, fz);
    else if (a.write_mask == 0)
        FW_LAUNCH_T((fw_k_update_fifo2<D, 0, 0>), grid, block, s, e0, e1, g, a, inl, fz);
    else
        FW_LAUNCH_T((fw_k_update_fifo2<D, -1, 0>), grid, block, s, e0, e1, g, a, inl, fz);
    return hipGetLastError();
}

hipError_t fw_launch_update_fifo2(hipStream_t s, const FwGlobals &g, const FwFifoArgs &a, const FwInlineOps &inl, const FwFuseArgs &fz,
                                  uint32_t total_tiles, int nt, hipEvent_t e0, hipEvent_t e1) {
    if (!total_tiles || !a.n_segs || !a.spinless || !a.q0pl || a.any_inst || a.small_tiles) return hipErrorInvalidValue;
    const dim3 grid(total_tiles), block(FW_BLOCK);
    static_assert(FW_FUSE_MAX == 8, "one instantiation per depth");
    switch (a.fused) {
    case 2: return fw_launch_fifo2_depth<2>(s, g, a, inl, fz, grid, block, nt, e0, e1);
    case 3: return fw_launch_fifo2_depth<3>(s, g, a, inl, fz, grid, block, nt, e0, e1);
    case 4: return fw_launch_fifo2_depth<4>(s, g, a, inl, fz, grid, block, nt, e0, e1);
    case 5: return fw_launch_fifo2_depth<5>(s, g, a, inl, fz, grid, block, nt, e0, e1);
    case 6: return fw_launch_fifo2_depth<6>(s, g, a, inl, fz, grid, block, nt, e0, e1);
    case 7: return fw_launch_fifo2_depth<7>(s, g, a, inl, fz, grid, block, nt, e0, e1);
    case 8: return fw_launch_fifo2_depth<8>(s, g, a, inl, fz, grid, block, nt, e0, e1);
    default: return hipErrorInvalidValue;
    }
}
