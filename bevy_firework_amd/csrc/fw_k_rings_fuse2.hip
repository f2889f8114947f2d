// fw_k_rings_fuse2.hip -- the FIFO ring kernel's forms that run SEVERAL frames of a spin-less launch in one pass (FwFifoArgs::fused = the
// depth, FwFuseArgs, fw_fuse2.h, DESIGN.md 4.0, rounds 22 to 24): fw_k_update_fifo2<D, WM, NT>, the FUSE arm of fw_update_fifo_body,
// instantiated here and nowhere else -- depths 2 to 8 over the four forms of the spin-less launch.  A unit of its own so that
// fw_k_rings.hip compiles to what it compiled to before the forms existed: the templates come from there.  Reached through
// fw_launch_update_fifo (fw_k_rings.hip), which routes every depth: this unit is one of the three behind that entry.
// One instantiation per depth, never a run-time depth: with the loops over FwFuseArgs left rolled the compiler indexes the by-value
// argument record dynamically and copies it to private memory -- 141 VGPRs, 1928 B of scratch per lane, three waves (round 24).  Every
// depth is launched: the default groups close at fw_ctx::fuse_depth, and a reader may flush a group of any depth from 2 to 7.
// (round 27: two sets of them.  This unit holds fw_k_update_fifo2, the forms in which "the spawning workgroups run no spin step" is a fact
// of the code -- FwFifoArgs::fuse_pad[FW_FIFO_NEWBORN] != 0, what the product launches; fw_k_rings_fuse2_eager.hip compiles the same
// lines with FW_FUSE2_EAGER into fw_k_update_fifo2_eager, the forms that spin what they spawn: the word is 0, FW_NEWBORN_SPIN=1.)
#ifndef FW_RINGS_TEMPLATES_ONLY
#define FW_RINGS_TEMPLATES_ONLY
#endif
#include "fw_k_rings.hip"
#ifdef FW_FUSE2_EAGER
#define FW_FUSE2_KERNEL fw_k_update_fifo2_eager
#define FW_FUSE2_LAUNCH fw_unit_update_fifo2_eager
#else
#define FW_FUSE2_KERNEL fw_k_update_fifo2
#define FW_FUSE2_LAUNCH fw_unit_update_fifo2
#endif

// (the forms of the spin-less launch: fw_launch_spinless_form, fw_k_rings.hip)
template <int D>
static hipError_t fw_launch_fifo2_depth(hipStream_t s, const FwGlobals &g, const FwFifoArgs &a, const FwInlineOps &inl, const FwFuseArgs &fz, dim3 grid,
                                        dim3 block, int nt, hipEvent_t e0, hipEvent_t e1) {
    return fw_launch_spinless_form(nt, a.write_mask, [&](auto WM, auto NT) {
        FW_LAUNCH_T((FW_FUSE2_KERNEL<D, decltype(WM)::value, decltype(NT)::value>), grid, block, s, e0, e1, g, a, inl, fz);
    });
}

hipError_t FW_FUSE2_LAUNCH(hipStream_t s, const FwGlobals &g, const FwFifoArgs &a, const FwInlineOps &inl, const FwFuseArgs &fz,
                           uint32_t total_tiles, int nt, hipEvent_t e0, hipEvent_t e1) {
    if (!total_tiles || !a.n_segs || !a.spinless || !a.q0pl || a.any_inst || a.small_tiles) return hipErrorInvalidValue;
#ifndef FW_FUSE2_EAGER
    if (a.fuse_pad[FW_FIFO_NEWBORN] == 0u) return fw_unit_update_fifo2_eager(s, g, a, inl, fz, total_tiles, nt, e0, e1);
#endif
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
