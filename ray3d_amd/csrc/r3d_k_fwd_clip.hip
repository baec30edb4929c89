// r3d_forward_clip_f32 / r3d_forward_clip_uv_f32: clip calls - first levels on the per-frame buffer (first_level_shared).
// One of the kernel translation units (r3d_tiles.hpp holds the tile code; r3d_kernels.hip the launchers that pick a kernel).
#include "r3d_tiles.hpp"

namespace r3d {

R3D_FORWARD_KERNEL(r3d_forward_clip_f32, false, false, false, true)
R3D_FORWARD_KERNEL(r3d_forward_clip_uv_f32, true, false, false, true)    // (UV input: GlobalInfo's current frames are still gathered)
FwdKernel fwd_kernel_clip(bool uv) { return uv ? r3d_forward_clip_uv_f32 : r3d_forward_clip_f32; }

}  // namespace r3d
