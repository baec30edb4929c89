// r3d_undistort_rays_f64: the pre-pass of R3D_INPUT_UV_DIST (include/ray3d_hip.h).  Pixel keypoints of a distorted camera
// in, float32 rays out - into the tail of the caller's workspace, where the R3D_INPUT_RAYS forward then reads them.  One
// keypoint per thread: its camera row (the row of the window the keypoint belongs to), the float64 routine of
// r3d_undistort.hpp (five fixed-point iterations, re-projection, encoding), one cast to float32 as
// lib/train_val/trainer.py:298 does.  Memory-streaming elementwise work: consecutive threads read consecutive 8-byte pixel
// pairs and write consecutive 12-byte rays; the camera rows (a few KiB for a batch) come from the caches.
#include "r3d_internal.hpp"
#include "r3d_undistort.hpp"

namespace r3d {

extern "C" __global__ __launch_bounds__(256) void r3d_undistort_rays_f64(const UndistArgs a) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.npts) return;
    int src = p, w;
    if (a.pts_per_window > 0) {              // materialised (B, RF, J, 3): window w's RF frames, read from the sliding input
        w = p / a.pts_per_window;
        src = w * a.window_stride * a.J + (p - w * a.pts_per_window);
    } else {                                 // one ray per input frame: frame f belongs to window min(f / stride, B - 1)
        w = min(p / a.J / a.window_stride, a.last_window);
    }
    const UndistRow k = undist_row(a.cam + (long long)w * a.cam_stride);
    const double u = (double)a.uv[2 * (long long)src], v = (double)a.uv[2 * (long long)src + 1];
    double uo, vo, r[3];
    undistort_pixel(k, u, v, uo, vo);
    pixel_to_ray(k, uo, vo, r);
    float *o = a.rays + 3 * (long long)p;
    o[0] = (float)r[0];
    o[1] = (float)r[1];
    o[2] = (float)r[2];
}

hipError_t launch_undistort(const UndistArgs &args, hipStream_t stream) {
    if (args.npts <= 0) return hipSuccess;
    r3d_undistort_rays_f64<<<dim3((args.npts + 255) / 256), dim3(256), 0, stream>>>(args);
    return hipGetLastError();
}

}  // namespace r3d
