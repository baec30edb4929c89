// r3d_forward_b3 / r3d_forward_uv_b3: the single-launch forward + the bf16x3 tiles (r3d_config.bf16x3, calls of >= 96 windows).
// One of the kernel translation units (r3d_tiles.hpp holds the tile code; r3d_kernels.hip the launchers that pick a kernel).
#include "r3d_tiles.hpp"

namespace r3d {

R3D_FORWARD_KERNEL(r3d_forward_b3, false, true, false, false)
R3D_FORWARD_KERNEL(r3d_forward_uv_b3, true, true, false, false)
FwdKernel fwd_kernel_b3(bool uv) { return uv ? r3d_forward_uv_b3 : r3d_forward_b3; }

}  // namespace r3d
