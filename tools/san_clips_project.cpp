// Stand-alone driver of r3d_debug_clips_project_host for `make san_clips_project` (ray3d_amd/csrc/Makefile): linked against
// libray3d_hip_san.so - the host objects built -fsanitize=address,undefined - and built with the same flags itself, it runs the
// argument checks, the descriptor rule and the per-point routines of r3d_clips_project on HOST memory only (no device call, no GPU
// needed).  Every buffer is an exact-size heap block (the sanitizer's red zones around it) whose first and last GUARD elements are
// a guard band of their own that must keep its fill: shuffled descriptors with gaps, several cameras on the same source frames,
// centred / causal / surplus padding, descriptors that end on the last row of a buffer, every kind of invalid descriptor, every
// combination of the optional outputs, all three encodings, non-finite points and a camera whose plane holds the points.
// Exit status 0: every result as expected and no sanitizer report.
#define R3D_TEST_HOOKS
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "ray3d_hip.h"

namespace {

int failures = 0;

void expect(bool ok, const char *what, int line) {
    if (!ok) {
        std::fprintf(stderr, "san_clips_project.cpp:%d: %s\n", line, what);
        ++failures;
    }
}
#define EXPECT(c) expect((c), #c, __LINE__)

float rnd(uint32_t &s) {
    s = s * 1664525u + 1013904223u;
    return (float)((s >> 8) & 0xffff) / 65536.0f - 0.5f;
}

constexpr float FILL = -7.0f;
constexpr int32_t COUNT0 = 1000;
constexpr size_t GUARD = 64;

// an exact-size heap block: GUARD elements of fill, the payload, GUARD elements of fill
template <class T> struct Banded {
    std::vector<T> mem;
    size_t n;
    T fill;
    Banded(size_t count, T f) : mem(count + 2 * GUARD, f), n(count), fill(f) {}
    T *data() { return mem.data() + GUARD; }
    T &operator[](size_t i) { return mem[GUARD + i]; }
    bool guards_clean() const {
        for (size_t i = 0; i < GUARD; ++i)
            if (std::memcmp(&mem[i], &fill, sizeof(T)) || std::memcmp(&mem[GUARD + n + i], &fill, sizeof(T))) return false;
        return true;
    }
};

struct Cam { double proj[12], cam[16], R[9], T[3]; };

Cam make_cam(uint32_t &seed, bool distorted) {
    Cam c;
    std::memset(&c, 0, sizeof(c));
    const double fx = 1145.0 + 10.0 * rnd(seed), fy = 1143.0 + 10.0 * rnd(seed), cx = 512.0 + 8.0 * rnd(seed), cy = 515.0 + 8.0 * rnd(seed);
    const double a = 0.4 * rnd(seed), ca = std::cos(a), sa = std::sin(a);
    // world -> camera: a rotation about x that turns z-up into y-down, then a yaw; the camera 5 m in front of the figure
    const double Rw2c[9] = {ca, sa, 0.0, 0.0, 0.0, -1.0, -sa, ca, 0.0}, t[3] = {0.1, 0.9, 5.0};
    const double K[9] = {fx, 0.0, cx, 0.0, fy, cy, 0.0, 0.0, 1.0};
    for (int r = 0; r < 3; ++r)
        for (int col = 0; col < 4; ++col) {
            double v = 0.0;
            for (int k = 0; k < 3; ++k) v += K[3 * r + k] * (col < 3 ? Rw2c[3 * k + col] : t[k]);
            c.proj[4 * r + col] = v;
        }
    const double p = 0.2 * rnd(seed);
    const double row[16] = {fx, fy, cx, cy, std::cos(p), std::sin(p), 1000.0, 1000.0, distorted ? -0.2 : 0.0, distorted ? 0.24 : 0.0,
                            distorted ? -0.0009 : 0.0, distorted ? -0.002 : 0.0, distorted ? -0.007 : 0.0, 0.0, 0.0, 0.0};
    std::memcpy(c.cam, row, sizeof(row));
    std::memcpy(c.R, Rw2c, sizeof(Rw2c));
    std::memcpy(c.T, t, sizeof(t));
    return c;
}

void run(int J, int encoding, bool mirror, bool with_gt, bool with_px, bool with_count) {
    const int F = encoding == R3D_ENCODE_RAY ? 3 : 2;
    const int64_t lengths[] = {1, 15, 16, 31}, gap = 3;
    const int src_order[] = {2, 0, 3, 1};
    int64_t src_first[4], total = 0;
    for (int i = 0; i < 4; ++i) {                                // no gap in front and none behind: clips touch both ends
        src_first[src_order[i]] = total;
        total += lengths[src_order[i]] + (i + 1 < 4 ? gap : 0);
    }
    uint32_t seed = 17u + (uint32_t)J * 3u + (uint32_t)encoding;
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    Banded<float> world((size_t)total * J * 3, nan);
    for (int c = 0; c < 4; ++c)
        for (int64_t i = 0; i < lengths[c] * J * 3; ++i) {
            const float v = rnd(seed);
            world[(size_t)(src_first[c] * J * 3 + i)] = i % 3 == 2 ? 0.9f + 1.7f * v : 0.7f * v;
        }
    const float special[] = {nan, inf, -inf, 3e38f, -3e38f, 1e-45f, -0.0f};
    for (int s = 0; s < 7; ++s) world[(size_t)((src_first[3] + 2 + s) * J + s % J) * 3 + s % 3] = special[s];
    Cam cams[3] = {make_cam(seed, false), make_cam(seed, true), make_cam(seed, false)};
    for (int k = 8; k < 12; ++k) cams[2].proj[k] = 0.0;          // camera 2: every point in its plane, h2 == 0
    // {source clip, camera, pad_front, pad_back}
    const int specs[][4] = {{0, 0, 4, 4}, {1, 1, 4, 4}, {2, 0, 4, 4}, {3, 1, 4, 4}, {2, 1, 8, 0}, {1, 0, 4, 5}, {3, 0, 4, 5}, {0, 2, 8, 0}, {2, 2, 4, 20}};
    const int k = 9, out_order[] = {4, 8, 1, 6, 0, 3, 7, 2, 5}, gt_order[] = {7, 2, 5, 0, 8, 3, 1, 6, 4};
    int64_t out_first[9], gt_first[9], out_rows = 0, gt_rows = 0, max_rows = 0;
    for (int i = 0; i < k; ++i) {
        const int o = out_order[i], g = gt_order[i];
        const int64_t rows = specs[o][2] + lengths[specs[o][0]] + specs[o][3];
        out_first[o] = out_rows;
        out_rows += rows + (i + 1 < k ? gap : 0);
        gt_first[g] = gt_rows;
        gt_rows += lengths[specs[g][0]] + (i + 1 < k ? gap : 0);
        if (rows > max_rows) max_rows = rows;
    }
    int32_t perm[17];
    for (int j = 0; j < J; ++j) perm[j] = J - 1 - j;
    const int64_t big = INT64_MAX;
    // invalid descriptors: {first_frame, n_frames, out_first, gt_first, pad_front, pad_back}; the gt kinds only in calls that write gt / px
    const int64_t bad[][6] = {{0, 0, 0, 0, 4, 4}, {0, 1, 0, 0, -1, 4}, {0, 1, 0, 0, 4, -1}, {0, 1, 0, 0, 4, (int)max_rows}, {total - 14, 15, 0, 0, 0, 0},
                              {-1, 1, 0, 0, 0, 0}, {0, 15, out_rows - 14, 0, 0, 0}, {0, 1, -1, 0, 0, 0}, {big, 1, 0, 0, 0, 0}, {0, big, 0, 0, 0, 0},
                              {0, 1, big, 0, 0, 0}, {0, 1, 0, 0, INT32_MAX, INT32_MAX}, {0, 15, 0, gt_rows - 14, 0, 0}, {0, 1, 0, -1, 0, 0},
                              {0, 1, 0, big, 0, 0}, {0, 1, 0, INT64_MIN, 0, 0}};
    const int nbad = (int)(sizeof(bad) / sizeof(bad[0])), first_gt_kind = 12;
    const bool has_gt = with_gt || with_px;
    std::vector<r3d_clip_project_desc> table;
    std::vector<int> kind;                                       // spec index, or -1 for an invalid descriptor
    for (int c = 0, b = 0; c < k; ++c) {
        r3d_clip_project_desc d;
        std::memset(&d, 0, sizeof(d));
        const Cam &cam = cams[specs[c][1]];
        d.first_frame = src_first[specs[c][0]];
        d.n_frames = lengths[specs[c][0]];
        d.out_first = out_first[c];
        d.gt_first = gt_first[c];
        d.pad_front = specs[c][2];
        d.pad_back = specs[c][3];
        std::memcpy(d.proj, cam.proj, sizeof(d.proj));
        std::memcpy(d.cam, cam.cam, sizeof(d.cam));
        std::memcpy(d.rw2g, cam.R, sizeof(d.rw2g));
        std::memcpy(d.tw2g, cam.T, sizeof(d.tw2g));
        table.push_back(d);
        kind.push_back(c);
        for (int r = 0; r < 2 && b < nbad; ++r, ++b) {
            if (b >= first_gt_kind && !has_gt) break;            // (without gt / px, gt_first is not read: those would be valid)
            r3d_clip_project_desc e = d;
            e.first_frame = bad[b][0];
            e.n_frames = bad[b][1];
            e.out_first = bad[b][2];
            e.gt_first = bad[b][3];
            e.pad_front = (int32_t)bad[b][4];
            e.pad_back = (int32_t)bad[b][5];
            table.push_back(e);
            kind.push_back(-1);
        }
    }
    const int nc = (int)table.size();
    Banded<float> x((size_t)out_rows * J * F, FILL), xm((size_t)out_rows * J * F, FILL), gt((size_t)gt_rows * J * 3, FILL);
    Banded<double> px((size_t)gt_rows * J * 2, (double)FILL);
    Banded<int32_t> outside((size_t)nc, COUNT0), status((size_t)nc, -1);
    const int rc = r3d_debug_clips_project_host(world.data(), total, J, encoding, table.data(), nc, max_rows, x.data(), out_rows,
                                                mirror ? xm.data() : nullptr, mirror ? perm : nullptr, with_gt ? gt.data() : nullptr,
                                                with_px ? px.data() : nullptr, gt_rows, with_count ? outside.data() : nullptr, status.data());
    EXPECT(rc == 0);
    EXPECT(world.guards_clean() && x.guards_clean() && xm.guards_clean() && gt.guards_clean() && px.guards_clean() && outside.guards_clean() &&
           status.guards_clean());
    std::vector<bool> out_cov((size_t)out_rows, false), gt_cov((size_t)gt_rows, false);
    for (int c = 0; c < nc; ++c) {
        EXPECT(status[(size_t)c] == (kind[(size_t)c] == -1 ? 1 : 0));
        if (kind[(size_t)c] == -1) {
            if (with_count) EXPECT(outside[(size_t)c] == COUNT0);
            continue;
        }
        const r3d_clip_project_desc &d = table[(size_t)c];
        const int64_t rows = d.pad_front + d.n_frames + d.pad_back;
        int32_t count = 0;
        for (int64_t r = 0; r < rows; ++r) {
            out_cov[(size_t)(d.out_first + r)] = true;
            int64_t f = r - d.pad_front;
            const bool body = f >= 0 && f < d.n_frames;
            f = f < 0 ? 0 : (f > d.n_frames - 1 ? d.n_frames - 1 : f);
            if (body && has_gt) gt_cov[(size_t)(d.gt_first + f)] = true;
            for (int j = 0; j < J; ++j) {
                const float *p = &world[(size_t)((d.first_frame + f) * J + j) * 3];
                double h[3];
                for (int i = 0; i < 3; ++i) h[i] = d.proj[4 * i] * p[0] + d.proj[4 * i + 1] * p[1] + d.proj[4 * i + 2] * p[2] + d.proj[4 * i + 3];
                const double u = h[0] / h[2], v = h[1] / h[2];
                const bool finite = std::isfinite(u) && std::isfinite(v);
                const bool out = !(u >= 0.0 && u <= 1000.0 && v >= 0.0 && v <= 1000.0);
                const float *e = &x[(size_t)((d.out_first + r) * J + j) * F];
                const float *m = &xm[(size_t)((d.out_first + r) * J + (J - 1 - j)) * F];      // perm is its own inverse
                for (int i = 0; i < F; ++i) {
                    if (!finite) { if (i == 0) EXPECT(!std::isfinite(e[0]) || !std::isfinite(e[1])); }
                    else EXPECT(std::isfinite(e[i]));
                    if (mirror) {
                        const float want = i == 0 ? -e[i] : e[i];
                        EXPECT(std::isnan(want) ? std::isnan(m[i]) : std::memcmp(&m[i], &want, 4) == 0);
                    }
                }
                if (finite && encoding == R3D_ENCODE_SCREEN) {
                    EXPECT(std::fabs((double)e[0] - (u / 1000.0 * 2 - 1)) <= 2e-7 * (1.0 + std::fabs(u) / 500.0));
                    EXPECT(std::fabs((double)e[1] - (v / 1000.0 * 2 - 1)) <= 2e-7 * (1.0 + std::fabs(v) / 500.0));
                }
                if (!body) continue;
                count += (out && kind[(size_t)c] >= 0) ? 1 : 0;
                const size_t at = (size_t)((d.gt_first + f) * J + j);
                if (with_px && kind[(size_t)c] >= 0) {
                    const double got[2] = {px[2 * at], px[2 * at + 1]}, want[2] = {u, v};
                    for (int i = 0; i < 2; ++i) {
                        if (std::isnan(want[i])) EXPECT(std::isnan(got[i]));
                        else if (!std::isfinite(want[i])) EXPECT(got[i] == want[i]);
                        else EXPECT(std::fabs(got[i] - want[i]) <= 1e-9 * (1.0 + std::fabs(want[i])));
                    }
                }
                if (with_gt && kind[(size_t)c] >= 0)
                    for (int i = 0; i < 3; ++i) {
                        const double ref = d.rw2g[3 * i] * p[0] + d.rw2g[3 * i + 1] * p[1] + d.rw2g[3 * i + 2] * p[2] + d.tw2g[i];
                        const float got = gt[3 * at + i];
                        if (!std::isfinite(ref)) EXPECT(!std::isfinite(got));
                        else EXPECT(std::fabs((double)got - ref) <= 2e-7 * (1.0 + std::fabs(ref)));
                    }
            }
        }
        if (with_count && kind[(size_t)c] >= 0) EXPECT(outside[(size_t)c] == COUNT0 + count);
    }
    for (int64_t r = 0; r < out_rows; ++r)
        for (int i = 0; i < J * F; ++i) {
            if (!out_cov[(size_t)r]) EXPECT(x[(size_t)(r * J * F + i)] == FILL);
            if (!out_cov[(size_t)r] || !mirror) EXPECT(xm[(size_t)(r * J * F + i)] == FILL);
        }
    for (int64_t r = 0; r < gt_rows; ++r) {
        for (int i = 0; i < J * 3; ++i)
            if (!gt_cov[(size_t)r] || !with_gt) EXPECT(gt[(size_t)(r * J * 3 + i)] == FILL);
        for (int i = 0; i < J * 2; ++i)
            if (!gt_cov[(size_t)r] || !with_px) EXPECT(px[(size_t)(r * J * 2 + i)] == (double)FILL);
    }
    // the argument rules: nothing may be written (status keeps what the valid call left)
    float *xo = x.data(), *mo = xm.data(), *go = gt.data();
    double *po = px.data();
    int32_t *oo = outside.data(), *so = status.data();
    const r3d_clip_project_desc *t = table.data();
    const std::vector<float> x_before = x.mem;
    const std::vector<int32_t> status_before = status.mem, outside_before = outside.mem;
    int32_t twice[17];
    for (int j = 0; j < J; ++j) twice[j] = 0;
#define CALL(W, TOT, JJ, ENC, TAB, NC, MR, X, OR, XM, PERM, GT, PX, GR) \
    EXPECT(r3d_debug_clips_project_host(W, TOT, JJ, ENC, TAB, NC, MR, X, OR, XM, PERM, GT, PX, GR, oo, so) == R3D_ERR_ARG)
    CALL(nullptr, total, J, encoding, t, nc, max_rows, xo, out_rows, mo, perm, go, po, gt_rows);
    CALL(world.data(), total, J, encoding, nullptr, nc, max_rows, xo, out_rows, mo, perm, go, po, gt_rows);
    CALL(world.data(), total, J, encoding, t, nc, max_rows, nullptr, out_rows, mo, perm, go, po, gt_rows);
    EXPECT(r3d_debug_clips_project_host(world.data(), total, J, encoding, t, nc, max_rows, xo, out_rows, mo, perm, go, po, gt_rows, oo, nullptr) == R3D_ERR_ARG);
    CALL(world.data(), total, J, encoding, t, 0, max_rows, xo, out_rows, mo, perm, go, po, gt_rows);
    CALL(world.data(), total, J, encoding, t, R3D_CLIPS_MAX + 1, max_rows, xo, out_rows, mo, perm, go, po, gt_rows);
    CALL(world.data(), total, 0, encoding, t, nc, max_rows, xo, out_rows, mo, perm, go, po, gt_rows);
    CALL(world.data(), total, 18, encoding, t, nc, max_rows, xo, out_rows, mo, perm, go, po, gt_rows);
    CALL(world.data(), total, J, 3, t, nc, max_rows, xo, out_rows, mo, perm, go, po, gt_rows);
    CALL(world.data(), total, J, encoding, t, nc, 0, xo, out_rows, mo, perm, go, po, gt_rows);
    CALL(world.data(), 0, J, encoding, t, nc, max_rows, xo, out_rows, mo, perm, go, po, gt_rows);
    CALL(world.data(), total, J, encoding, t, nc, max_rows, xo, 0, mo, perm, go, po, gt_rows);
    CALL(world.data(), total, J, encoding, t, nc, (int64_t)R3D_ENCODE_MAX_POINTS / J + 1, xo, out_rows, mo, perm, go, po, gt_rows);
    CALL(world.data(), (int64_t)R3D_ENCODE_MAX_POINTS + 1, J, encoding, t, nc, max_rows, xo, out_rows, mo, perm, go, po, gt_rows);
    CALL(world.data(), total, J, encoding, t, nc, max_rows, xo, (int64_t)R3D_ENCODE_MAX_POINTS + 1, mo, perm, go, po, gt_rows);
    CALL(world.data(), total, J, encoding, t, nc, max_rows, xo, out_rows, nullptr, perm, go, po, gt_rows);
    CALL(world.data(), total, J, encoding, t, nc, max_rows, xo, out_rows, mo, nullptr, go, po, gt_rows);
    if (J > 1) CALL(world.data(), total, J, encoding, t, nc, max_rows, xo, out_rows, mo, twice, go, po, gt_rows);
    CALL(world.data(), total, J, encoding, reinterpret_cast<const r3d_clip_project_desc *>(reinterpret_cast<const char *>(t) + 4), nc, max_rows, xo,
         out_rows, mo, perm, go, po, gt_rows);
    CALL(world.data(), total, J, encoding, t, nc, max_rows, xo, out_rows, mo, perm, go, po, 0);
    CALL(world.data(), total, J, encoding, t, nc, max_rows, xo, out_rows, mo, perm, go, nullptr, -1);
    CALL(world.data(), total, J, encoding, t, nc, max_rows, xo, out_rows, mo, perm, nullptr, po, (int64_t)R3D_ENCODE_MAX_POINTS + 1);
    CALL(world.data(), total, J, encoding, t, nc, max_rows, xo, out_rows, mo, perm, go, reinterpret_cast<double *>(reinterpret_cast<char *>(po) + 4), gt_rows);
#undef CALL
    EXPECT(x.mem == x_before || std::memcmp(x.mem.data(), x_before.data(), x_before.size() * sizeof(float)) == 0);
    EXPECT(status.mem == status_before && outside.mem == outside_before);
}

}  // namespace

int main() {
    for (int J : {1, 14, 17})
        for (int encoding : {R3D_ENCODE_RAY, R3D_ENCODE_INTRINSIC, R3D_ENCODE_SCREEN})
            for (int m = 0; m < 16; ++m) run(J, encoding, m & 1, m & 2, m & 4, m & 8);
    if (failures) {
        std::fprintf(stderr, "%d expectation(s) failed\n", failures);
        return 1;
    }
    std::printf("san_clips_project: ok\n");
    return 0;
}
