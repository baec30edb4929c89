// R3D_INPUT_UV_DIST / R3D_INPUT_PX_INTRINSIC / R3D_INPUT_PX_SCREEN: the per-keypoint arithmetic of the pixel pre-pass
// (r3d_k_elementwise.hip), __host__ __device__ so that the hooks build runs the very same routines on the CPU
// (r3d_debug_undistort_host, r3d_debug_encode_px_host, r3d_debug_clips_encode_host).  float64 throughout, in the reference's order
// (lib/camera/camera.py:412-441): cv2.undistortPoints(uv, K, dist, P=K) - five fixed-point iterations of OpenCV's
// documented algorithm for the 5-coefficient Brown-Conrady model, then re-projection with K - followed by one of three
// encodings: the ray of get_cam_ray_given_uv (:460-471), the two components of encode_uv_with_intrinsic (:438-439), or -
// without the undistortion, the reference normalises raw pixels - normalize_screen_coordinates (:11-18).  PARITY UNPINNED
// against cv2 itself (OpenCV is not a dependency of this project); pinned against the restatements in
// ray3d_amd/camera.py, oracle.undistort_points and tests/golden/undistort.npz; the two 2-float encodings are pinned to the
// reference's own values (tests/golden/px2d.npz).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace r3d {

// A camera row of the pre-pass: {fx, fy, cx, cy, cos(pitch), sin(pitch), res_w, res_h, k1, k2, p1, p2, k3, 0, 0, 0}.
// Slots 6 / 7 (the image's width and height in pixels; 0 when unknown) are read by the screen encoding ONLY - the other two
// never touch them; cos / sin are read by the ray encoding only.
constexpr int UNDIST_ROW_DOUBLES = 16;
constexpr int UNDIST_ROW_RES_W = 6, UNDIST_ROW_RES_H = 7;

// What the pre-pass writes per keypoint (UndistArgs::encoding, uniform over a launch)
constexpr int ENC_RAY = 0;        // 3 floats: the ray (R3D_INPUT_UV_DIST)
constexpr int ENC_INTRINSIC = 1;  // 2 floats: ((u-cx)/fx, (v-cy)/fy) of the undistorted pixel (R3D_INPUT_PX_INTRINSIC)
constexpr int ENC_SCREEN = 2;     // 2 floats: (u/w*2 - 1, v/w*2 - h/w) of the raw pixel (R3D_INPUT_PX_SCREEN)
__host__ __device__ inline int enc_floats(int encoding) { return encoding == ENC_RAY ? 3 : 2; }

struct UndistRow { double fx, fy, cx, cy, c, s, k1, k2, p1, p2, k3; };

__host__ __device__ inline UndistRow undist_row(const double *r) {
    return UndistRow{r[0], r[1], r[2], r[3], r[4], r[5], r[8], r[9], r[10], r[11], r[12]};
}

// All five coefficients zero: the reference's undistort=False - no iteration, no re-projection (bit-identical to UV mode)
__host__ __device__ inline bool undist_identity(const UndistRow &k) {
    return k.k1 == 0.0 && k.k2 == 0.0 && k.p1 == 0.0 && k.p2 == 0.0 && k.k3 == 0.0;
}

// Pixel (u, v) with the lens distortion removed, in pixels (Camera.undistort_points of ray3d_amd/camera.py, term for term).
// Divisions are IEEE (correctly rounded) in both compilations: no reciprocal approximations.
__host__ __device__ inline void undistort_pixel(const UndistRow &k, double u, double v, double &uo, double &vo) {
    if (undist_identity(k)) { uo = u; vo = v; return; }
    const double x0 = (u - k.cx) / k.fx, y0 = (v - k.cy) / k.fy;
    double x = x0, y = y0;
    for (int it = 0; it < 5; ++it) {
        const double r2 = x * x + y * y;
        const double icd = 1.0 / (1 + ((k.k3 * r2 + k.k2) * r2 + k.k1) * r2);
        const double dx = 2 * k.p1 * x * y + k.p2 * (r2 + 2 * x * x);
        const double dy = k.p1 * (r2 + 2 * y * y) + 2 * k.p2 * x * y;
        x = (x0 - dx) * icd;
        y = (y0 - dy) * icd;
    }
    uo = x * k.fx + k.cx;                   // re-projection with P = K
    vo = y * k.fy + k.cy;
}

// The intrinsic encoding of an (undistorted) pixel: ((u-cx)/fx, (v-cy)/fy) - encode_uv_with_intrinsic's two components
// (camera.py:438-439; pp_cam is the principal point), IEEE subtraction and division.
__host__ __device__ inline void pixel_to_intrinsic(const UndistRow &k, double u, double v, double o[2]) {
    o[0] = (u - k.cx) / k.fx;
    o[1] = (v - k.cy) / k.fy;
}

// The ray of an (undistorted) pixel: (x, c*y+s, -s*y+c) with (x, y) the intrinsic encoding - the expressions of uv_to_ray
// (r3d_tiles.hpp), so that zero coefficients give UV mode's values bit for bit.
__host__ __device__ inline void intrinsic_to_ray(const UndistRow &k, const double o[2], double r[3]) {
    const double tx = o[0], t = o[1];
    r[0] = tx;
    r[1] = k.c * t + k.s;
    r[2] = -k.s * t + k.c;
}
__host__ __device__ inline void pixel_to_ray(const UndistRow &k, double u, double v, double r[3]) {
    double o[2];
    pixel_to_intrinsic(k, u, v, o);
    intrinsic_to_ray(k, o, r);
}

// The screen encoding of a RAW pixel in a w x h image: X / w * 2 - [1, h / w] (normalize_screen_coordinates,
// camera.py:11-18) in that operation order.  (A compiler may contract "x * 2 - c" into one fma: the product by 2 is exact,
// so the fused and the two-step forms round the same exact value - the result does not depend on it.)
__host__ __device__ inline void pixel_to_screen(double w, double h, double u, double v, double o[2]) {
    o[0] = u / w * 2 - 1;
    o[1] = v / w * 2 - h / w;
}

// One keypoint through the 2-float encodings (ENC_INTRINSIC / ENC_SCREEN) from its 16-double camera row
__host__ __device__ inline void encode_pixel_2d(const double *row, int encoding, double u, double v, double o[2]) {
    if (encoding == ENC_SCREEN) {
        pixel_to_screen(row[UNDIST_ROW_RES_W], row[UNDIST_ROW_RES_H], u, v, o);
        return;
    }
    const UndistRow k = undist_row(row);
    double uo, vo;
    undistort_pixel(k, u, v, uo, vo);
    pixel_to_intrinsic(k, uo, vo, o);
}

// One keypoint through the encoding `encoding` from its 16-double camera row, cast ONCE to float32 (z: ENC_RAY only, 0
// otherwise): what r3d_undistort_rays_f64 (the forwards' pre-pass) and r3d_k_clips_encode (r3d_clips_encode) write per point, and
// what the hooks' r3d_debug_clips_encode_host writes on the CPU.  `encoding` is uniform over a launch: scalar branches.  (Values,
// not an output array: nothing of it lives in scratch memory.)
struct EncodedPoint { float x, y, z; };
// The one cast.  A NaN (a bad pixel coordinate) leaves as THE canonical quiet NaN: which operand's sign and payload a NaN result
// carries differs between the GPU and a host CPU, and the kernel and the host hook are held to the same bits.
__host__ __device__ __forceinline__ float encoded_f32(const double d) {
    return d != d ? __builtin_bit_cast(float, 0x7fc00000u) : (float)d;
}
__host__ __device__ __forceinline__ EncodedPoint encode_point_f32(const double *row, int encoding, double u, double v) {
    double e[2], z = 0.0;
    if (encoding == ENC_SCREEN) {            // raw pixels and the image size: no undistortion, no intrinsics
        pixel_to_screen(row[UNDIST_ROW_RES_W], row[UNDIST_ROW_RES_H], u, v, e);
    } else {
        const UndistRow k = undist_row(row);
        double uo, vo;
        undistort_pixel(k, u, v, uo, vo);
        pixel_to_intrinsic(k, uo, vo, e);    // (shared: the ray's first component and the argument of the other two)
        if (encoding != ENC_INTRINSIC) {
            double r[3];
            intrinsic_to_ray(k, e, r);
            e[0] = r[0];
            e[1] = r[1];
            z = r[2];
        }
    }
    return EncodedPoint{encoded_f32(e[0]), encoded_f32(e[1]), encoded_f32(z)};
}

// ---- r3d_clips_encode: the descriptor rules and the row-to-source mapping, shared by the kernel and the host hook ----

// A descriptor the call follows (include/ray3d_hip.h: "invalid descriptors", written so that no sum can overflow): at least
// one frame, no negative pad, pad_front + n + pad_back <= max_rows, the source frames inside [0, total_frames), the output
// rows inside [0, out_rows).
__host__ __device__ inline bool clip_input_valid(long long first, long long n, long long out_first, int pad_front, int pad_back,
                                                 long long total_frames, long long out_rows, long long max_rows) {
    if (n < 1 || pad_front < 0 || pad_back < 0 || n > max_rows) return false;
    const long long pads = (long long)pad_front + pad_back;
    if (pads > max_rows - n) return false;
    if (first < 0 || n > total_frames || first > total_frames - n) return false;
    const long long rows = n + pads;
    return out_first >= 0 && rows <= out_rows && out_first <= out_rows - rows;
}

// Output row r of a clip repeats source frame clamp(r - pad_front, 0, n - 1): np.pad(..., 'edge') (generators.py:213-216)
__host__ __device__ inline long long clip_input_source(long long r, int pad_front, long long n) {
    const long long f = r - pad_front;
    return f < 0 ? 0 : (f > n - 1 ? n - 1 : f);
}

// The mirrored copy writes point j of the plain buffer to point inv[j] (the inverse of mirror_perm), 5 bits per joint, 12
// joints per word - kernel arguments, like the parent table of the validation losses.
__host__ __device__ inline int mirror_dest(unsigned long long w0, unsigned long long w1, int j) {
    return (int)((j < 12 ? w0 >> (5 * j) : w1 >> (5 * (j - 12))) & 31ull);
}
// mirror_perm (J entries, a permutation of 0..J-1: the caller checked) -> its packed inverse
inline void mirror_pack_inverse(const int32_t *perm, int J, unsigned long long w[2]) {
    w[0] = w[1] = 0ull;
    for (int j = 0; j < J; ++j) {
        const int src = perm[j];             // x_mirror[row, j] = x[row, src]: the thread of point src writes to j
        w[src < 12 ? 0 : 1] |= (unsigned long long)j << (5 * (src < 12 ? src : src - 12));
    }
}

}  // namespace r3d
