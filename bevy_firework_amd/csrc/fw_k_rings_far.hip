// fw_k_rings_far.hip -- the far tier of the fused FIFO ring kernel (round 32): fw_k_update_fifo_far<D, WM, NT>, the FUSE arm
// of fw_update_fifo_body at depths FW_FUSE_MAX + 1 .. FW_FUSE_FAR (9 to 16) over the four forms of the spin-less launch.  A unit of its own,
// like fw_k_rings_fuse2.hip and for the same reason: fw_k_rings.hip and the first tier's units compile to what they compiled to; the
// templates come from fw_k_rings.hip, and so does the one entry that routes a launch of these depths here (fw_launch_update_fifo).  One
// instantiation per depth, never a run-time depth (fw_k_rings_fuse2.hip says why), and every depth is launched: the default groups close at fw_ctx::fuse_far_depth, and a reader may flush a far group of any depth up to FW_FUSE_FAR - 1.
// What a far kernel knows beside the first tier's arguments is its FIFTH argument, FwFarArgs: dt and boundaries of withheld frames
// FW_FUSE_MAX - 1 .. D - 2; the body picks the record by the frame's index (dt_w, spawn_end_w, dead_w).
// NBFACT forms only -- the spawning workgroups defer the spin of what they spawn, what the product launches: under FW_NEWBORN_SPIN=1 the
// host keeps its groups at FW_FUSE_MAX (launch_fifo) and a launch that says otherwise is refused here.
#ifndef FW_RINGS_TEMPLATES_ONLY
#define FW_RINGS_TEMPLATES_ONLY
#endif
#include "fw_k_rings.hip"

// (the forms of the spin-less launch: fw_launch_spinless_form, fw_k_rings.hip)
template <int D>
static hipError_t fw_launch_fifo_far_depth(hipStream_t s, const FwGlobals &g, const FwFifoArgs &a, const FwInlineOps &inl, const FwFuseArgs &fz, const FwFarArgs &far,
                                           dim3 grid, dim3 block, int nt, hipEvent_t e0, hipEvent_t e1) {
    return fw_launch_spinless_form(nt, a.write_mask, [&](auto WM, auto NT) {
        FW_LAUNCH_T((fw_k_update_fifo_far<D, decltype(WM)::value, decltype(NT)::value>), grid, block, s, e0, e1, g, a, inl, fz, far);
    });
}

hipError_t fw_unit_update_fifo_far(hipStream_t s, const FwGlobals &g, const FwFifoArgs &a, const FwInlineOps &inl, const FwFuseArgs &fz,
                                   const FwFarArgs &far, uint32_t total_tiles, int nt, hipEvent_t e0, hipEvent_t e1) {
    if (!total_tiles || !a.n_segs || !a.spinless || !a.q0pl || a.any_inst || a.small_tiles || a.any_coll || a.n_nest) return hipErrorInvalidValue;
    if (a.fuse_pad[FW_FIFO_NEWBORN] == 0u) return hipErrorInvalidValue;  // (no eager forms in this tier)
    const dim3 grid(total_tiles), block(FW_BLOCK);
    static_assert(FW_FUSE_MAX == 8 && FW_FUSE_FAR == 16, "one instantiation per depth");
    switch (a.fused) {
    case 9: return fw_launch_fifo_far_depth<9>(s, g, a, inl, fz, far, grid, block, nt, e0, e1);
    case 10: return fw_launch_fifo_far_depth<10>(s, g, a, inl, fz, far, grid, block, nt, e0, e1);
    case 11: return fw_launch_fifo_far_depth<11>(s, g, a, inl, fz, far, grid, block, nt, e0, e1);
    case 12: return fw_launch_fifo_far_depth<12>(s, g, a, inl, fz, far, grid, block, nt, e0, e1);
    case 13: return fw_launch_fifo_far_depth<13>(s, g, a, inl, fz, far, grid, block, nt, e0, e1);
    case 14: return fw_launch_fifo_far_depth<14>(s, g, a, inl, fz, far, grid, block, nt, e0, e1);
    case 15: return fw_launch_fifo_far_depth<15>(s, g, a, inl, fz, far, grid, block, nt, e0, e1);
    case 16: return fw_launch_fifo_far_depth<16>(s, g, a, inl, fz, far, grid, block, nt, e0, e1);
    default: return hipErrorInvalidValue;
    }
}
