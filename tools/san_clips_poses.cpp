// Stand-alone driver of r3d_debug_clips_poses_host for `make san_clips_poses` (ray3d_amd/csrc/Makefile): linked against
// libray3d_hip_san.so - the host objects built -fsanitize=address,undefined - and built with the same flags itself, it runs the
// argument checks, the descriptor rule and the per-point routines of r3d_clips_poses on HOST memory only (no device call, no GPU
// needed) over exact-size heap buffers: shuffled clips with gaps and surplus rows, clips that end on the last row of a buffer,
// every kind of invalid descriptor, with and without the mirrored pass, pred only / world only / both, non-finite values.
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
        std::fprintf(stderr, "san_clips_poses.cpp:%d: %s\n", line, what);
        ++failures;
    }
}
#define EXPECT(c) expect((c), #c, __LINE__)

float rnd(uint32_t &s) {
    s = s * 1664525u + 1013904223u;
    return (float)((s >> 8) & 0xffff) / 65536.0f - 0.5f;
}

constexpr float FILL = -7.0f;

void run(int J, bool mirror, bool with_pred, bool with_world) {
    const int64_t lengths[] = {1, 2, 15, 16, 40, 257}, surplus[] = {0, 2, 1, 0, 24, 127}, gap = 3;
    const int order_raw[] = {3, 0, 5, 1, 4, 2}, order_out[] = {2, 5, 1, 4, 0, 3};
    const int k = 6;
    int64_t first[6], raw_at[6], total = 0, raw_rows = 0;       // no gap in front and none behind: the first and the last clip touch the ends
    for (int i = 0; i < k; ++i) {
        raw_at[order_raw[i]] = raw_rows;
        raw_rows += lengths[order_raw[i]] + surplus[order_raw[i]] + (i + 1 < k ? gap : 0);
        first[order_out[i]] = total;
        total += lengths[order_out[i]] + (i + 1 < k ? gap : 0);
    }
    raw_rows -= surplus[order_raw[k - 1]];                       // the last stored clip ends on the last raw row
    uint32_t seed = 11u + (uint32_t)J;
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::vector<float> raw((size_t)raw_rows * J * 3), raw_m((size_t)raw_rows * J * 3);
    for (auto &v : raw) v = rnd(seed);
    for (auto &v : raw_m) v = rnd(seed);
    const float special[] = {nan, inf, -inf, 3e38f, -3e38f, 1e-45f, -0.0f};
    for (int s = 0; s < 7; ++s) {
        raw[(size_t)((raw_at[4] + s) * J + s % J) * 3 + s % 3] = special[s];
        raw_m[(size_t)((raw_at[4] + 8 + s) * J + s % J) * 3 + s % 3] = special[s];
    }
    int32_t perm[17];
    for (int j = 0; j < J; ++j) perm[j] = J - 1 - j;
    // valid clips with an invalid descriptor between any two: {first_frame, n_frames, raw_first}
    const int64_t big = INT64_MAX;
    const int64_t bad[][3] = {{5, 0, 0}, {0, 258, 0}, {total - 15, 16, 0}, {-1, 4, 0}, {0, 4, -1}, {0, 16, raw_rows - 15}, {big, 3, 0}, {0, 3, big},
                              {0, big, 0}, {total, 1, 0}, {0, 1, raw_rows}, {INT64_MIN, 2, INT64_MIN}};
    const int nbad = (int)(sizeof(bad) / sizeof(bad[0]));
    std::vector<r3d_clip_desc> table;
    std::vector<int64_t> raw_first;
    std::vector<int> kind;                                       // clip index, or -1 for an invalid descriptor
    for (int c = 0, b = 0; c < k; ++c) {
        r3d_clip_desc d;
        std::memset(&d, 0, sizeof(d));
        d.first_frame = first[c];
        d.n_frames = lengths[c];
        for (int i = 0; i < 9; ++i) d.rn2w[i] = (double)rnd(seed);
        for (int i = 0; i < 3; ++i) d.tn2w[i] = (double)rnd(seed) * 4.0;
        table.push_back(d);
        raw_first.push_back(raw_at[c]);
        kind.push_back(c);
        for (int r = 0; r < 2 && b < nbad; ++r, ++b) {
            r3d_clip_desc e = d;
            e.first_frame = bad[b][0];
            e.n_frames = bad[b][1];
            table.push_back(e);
            raw_first.push_back(bad[b][2]);
            kind.push_back(-1);
        }
    }
    const int nc = (int)table.size();
    std::vector<float> pred((size_t)total * J * 3, FILL);
    std::vector<double> world((size_t)total * J * 3, (double)FILL);
    std::vector<int32_t> status((size_t)nc, -1);
    const int rc = r3d_debug_clips_poses_host(raw.data(), mirror ? raw_m.data() : nullptr, raw_rows, J, mirror ? perm : nullptr, table.data(),
                                              raw_first.data(), nc, 257, with_pred ? pred.data() : nullptr, with_world ? world.data() : nullptr,
                                              total, status.data());
    EXPECT(rc == 0);
    std::vector<bool> covered((size_t)total, false);
    for (int c = 0; c < nc; ++c) {
        EXPECT(status[(size_t)c] == (kind[(size_t)c] < 0 ? 1 : 0));
        if (kind[(size_t)c] < 0) continue;
        const r3d_clip_desc &d = table[(size_t)c];
        for (int64_t f = 0; f < d.n_frames; ++f) {
            covered[(size_t)(d.first_frame + f)] = true;
            for (int j = 0; j < J; ++j) {
                float p[3];
                const float *r = &raw[(size_t)((raw_first[(size_t)c] + f) * J + j) * 3];
                const float *m = &raw_m[(size_t)((raw_first[(size_t)c] + f) * J + perm[j]) * 3];
                for (int i = 0; i < 3; ++i) {
                    volatile float s = r[i] + (i == 0 ? -m[i] : m[i]);     // (volatile: one float32 rounding each)
                    volatile float h = s * 0.5f;
                    p[i] = mirror ? h : r[i];
                }
                const size_t at = (size_t)((d.first_frame + f) * J + j) * 3;
                bool finite = true;
                for (int i = 0; i < 3; ++i) {
                    finite = finite && std::isfinite(p[i]);
                    if (with_pred) EXPECT(std::isnan(p[i]) ? std::isnan(pred[at + i]) : std::memcmp(&pred[at + i], &p[i], 4) == 0);
                }
                for (int i = 0; i < 3 && with_world; ++i) {
                    const double w = world[at + i];
                    if (!finite) { EXPECT(!std::isfinite(w)); continue; }
                    const double *R = &d.rn2w[3 * i];
                    const double ref = R[0] * p[0] + R[1] * p[1] + R[2] * p[2] + d.tn2w[i];
                    const double mag = std::fabs(R[0] * p[0]) + std::fabs(R[1] * p[1]) + std::fabs(R[2] * p[2]) + std::fabs(d.tn2w[i]);
                    EXPECT(std::fabs(w - ref) <= 8.0 * 0x1p-53 * mag);
                }
            }
        }
    }
    for (int64_t f = 0; f < total; ++f)
        for (int i = 0; i < J * 3; ++i) {
            if (!covered[(size_t)f] || !with_pred) EXPECT(pred[(size_t)(f * J * 3 + i)] == FILL);
            if (!covered[(size_t)f] || !with_world) EXPECT(world[(size_t)(f * J * 3 + i)] == (double)FILL);
        }
    // the argument rules: both outputs null, one of the mirror pair, a bad permutation, counts, in-place use
    float *po = pred.data();
    double *wo = world.data();
    EXPECT(r3d_debug_clips_poses_host(raw.data(), nullptr, raw_rows, J, nullptr, table.data(), raw_first.data(), nc, 257, nullptr, nullptr, total,
                                      status.data()) == R3D_ERR_ARG);
    EXPECT(r3d_debug_clips_poses_host(raw.data(), raw_m.data(), raw_rows, J, nullptr, table.data(), raw_first.data(), nc, 257, po, wo, total,
                                      status.data()) == R3D_ERR_ARG);
    EXPECT(r3d_debug_clips_poses_host(raw.data(), nullptr, raw_rows, J, perm, table.data(), raw_first.data(), nc, 257, po, wo, total,
                                      status.data()) == R3D_ERR_ARG);
    int32_t twice[17];
    for (int j = 0; j < J; ++j) twice[j] = 0;
    if (J > 1)
        EXPECT(r3d_debug_clips_poses_host(raw.data(), raw_m.data(), raw_rows, J, twice, table.data(), raw_first.data(), nc, 257, po, wo, total,
                                          status.data()) == R3D_ERR_ARG);
    EXPECT(r3d_debug_clips_poses_host(raw.data(), nullptr, raw_rows, J, nullptr, table.data(), raw_first.data(), 0, 257, po, wo, total,
                                      status.data()) == R3D_ERR_ARG);
    EXPECT(r3d_debug_clips_poses_host(raw.data(), nullptr, raw_rows, 18, nullptr, table.data(), raw_first.data(), nc, 257, po, wo, total,
                                      status.data()) == R3D_ERR_ARG);
    EXPECT(r3d_debug_clips_poses_host(raw.data(), nullptr, raw_rows, J, nullptr, table.data(), raw_first.data(), nc, 0, po, wo, total,
                                      status.data()) == R3D_ERR_ARG);
    EXPECT(r3d_debug_clips_poses_host(raw.data(), nullptr, raw_rows, J, nullptr, table.data(), raw_first.data(), nc, 257, raw.data() + 3, nullptr,
                                      raw_rows - 1, status.data()) == R3D_ERR_ARG);
    EXPECT(r3d_debug_clips_poses_host(raw.data(), raw_m.data(), raw_rows, J, perm, table.data(), raw_first.data(), nc, 257, raw_m.data(), nullptr,
                                      raw_rows, status.data()) == R3D_ERR_ARG);
}

}  // namespace

int main() {
    for (int J : {1, 14, 17})
        for (int m = 0; m < 8; ++m) {
            if (!(m & 2) && !(m & 4)) continue;                  // (both outputs null is an argument error: checked inside run)
            run(J, m & 1, m & 2, m & 4);
        }
    if (failures) {
        std::fprintf(stderr, "%d expectation(s) failed\n", failures);
        return 1;
    }
    std::printf("san_clips_poses: ok\n");
    return 0;
}
