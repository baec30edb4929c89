// r3d_undistort_rays_f64: the pixel pre-pass of R3D_INPUT_UV_DIST, R3D_INPUT_PX_INTRINSIC and R3D_INPUT_PX_SCREEN
// (include/ray3d_hip.h).  Raw pixel keypoints in, the model's float32 input out - into the tail of the caller's workspace,
// where the R3D_INPUT_RAYS forward then reads it.  One keypoint per thread: its camera row (the row of the window the
// keypoint belongs to), the float64 routines of r3d_undistort.hpp, one cast to float32 as lib/train_val/trainer.py:298
// does.  `encoding` (uniform over the launch: scalar branches around the shared arithmetic) selects what is written:
//   ENC_RAY        five fixed-point iterations, re-projection, the 3-float ray (the kernel's name dates from this one);
//   ENC_INTRINSIC  the same undistortion, then the 2 floats ((u-cx)/fx, (v-cy)/fy) - the 2-feature models' input under
//                  INTRINSIC_ENCODING;
//   ENC_SCREEN     no undistortion: the 2 floats (u/w*2 - 1, v/w*2 - h/w) from the row's resolution slots.
// Memory-streaming elementwise work: consecutive threads read consecutive 8-byte pixel pairs and write consecutive 12-
// or 8-byte outputs; the camera rows (a few KiB for a batch) come from the caches.
#include "r3d_internal.hpp"
#include "r3d_undistort.hpp"

namespace r3d {

extern "C" __global__ __launch_bounds__(256) void r3d_undistort_rays_f64(const UndistArgs a) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.npts) return;
    int src = p, w;
    if (a.pts_per_window > 0) {              // materialised (B, RF, J, F): window w's RF frames, read from the sliding input
        w = p / a.pts_per_window;
        src = w * a.window_stride * a.J + (p - w * a.pts_per_window);
    } else {                                 // one point per input frame: frame f belongs to window min(f / stride, B - 1)
        w = min(p / a.J / a.window_stride, a.last_window);
    }
    const double *row = a.cam + (long long)w * a.cam_stride;
    const double u = (double)a.uv[2 * (long long)src], v = (double)a.uv[2 * (long long)src + 1];
    if (a.encoding == ENC_SCREEN) {          // raw pixels and the image size: no undistortion, no intrinsics
        double e[2];
        pixel_to_screen(row[UNDIST_ROW_RES_W], row[UNDIST_ROW_RES_H], u, v, e);
        float *o = a.rays + 2 * (long long)p;
        o[0] = (float)e[0];
        o[1] = (float)e[1];
        return;
    }
    const UndistRow k = undist_row(row);
    double uo, vo, e[2], r[3];
    undistort_pixel(k, u, v, uo, vo);
    pixel_to_intrinsic(k, uo, vo, e);        // (shared: the ray's first component and the argument of the other two)
    if (a.encoding == ENC_INTRINSIC) {
        float *o = a.rays + 2 * (long long)p;
        o[0] = (float)e[0];
        o[1] = (float)e[1];
        return;
    }
    intrinsic_to_ray(k, e, r);
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
