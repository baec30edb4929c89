// r3d_forward_f32 / r3d_forward_uv_f32: the single-launch forward with the fp32 throughput tiles only (the headline kernel).
// One of the kernel translation units (r3d_tiles.hpp holds the tile code; r3d_kernels.hip the launchers that pick a kernel).
#include "r3d_tiles.hpp"

namespace r3d {

R3D_FORWARD_KERNEL(r3d_forward_f32, false, false, false, false)
R3D_FORWARD_KERNEL(r3d_forward_uv_f32, true, false, false, false)
FwdKernel fwd_kernel_f32(bool uv) { return uv ? r3d_forward_uv_f32 : r3d_forward_f32; }

}  // namespace r3d
