// r3d_forward_lat / r3d_forward_uv_lat: the single-launch forward + GEMV / latency tiles (calls of <= 32 windows).
// One of the kernel translation units (r3d_tiles.hpp holds the tile code; r3d_kernels.hip the launchers that pick a kernel).
#include "r3d_tiles.hpp"

namespace r3d {

R3D_FORWARD_KERNEL(r3d_forward_lat, false, false, true, false)
R3D_FORWARD_KERNEL(r3d_forward_uv_lat, true, false, true, false)
FwdKernel fwd_kernel_lat(bool uv) { return uv ? r3d_forward_uv_lat : r3d_forward_lat; }

}  // namespace r3d
