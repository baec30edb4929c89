// Stand-alone driver of r3d_debug_clips_valid_losses_host for `make san_clips_valid` (ray3d_amd/csrc/Makefile): linked against
// libray3d_hip_san.so - the host objects built -fsanitize=address,undefined - and built with the same flags itself, it runs the
// argument checks, the descriptor rule and the per-clip host routine on HOST memory only (no device call, no GPU needed) over
// exact-size heap buffers: shuffled clips with gaps, every kind of invalid descriptor, strided rows, with and without a
// trajectory, a parent table and a frame table.  Exit status 0: every result as expected and no sanitizer report.
#define R3D_TEST_HOOKS
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ray3d_hip.h"

namespace {

int failures = 0;

void expect(bool ok, const char *what, int line) {
    if (!ok) {
        std::fprintf(stderr, "san_clips_valid.cpp:%d: %s\n", line, what);
        ++failures;
    }
}
#define EXPECT(c) expect((c), #c, __LINE__)

float rnd(uint32_t &s) {
    s = s * 1664525u + 1013904223u;
    return (float)((s >> 8) & 0xffff) / 65536.0f - 0.5f;
}

bool same_bits(const double *a, const double *b, size_t n) { return std::memcmp(a, b, n * sizeof(double)) == 0; }

void run(int J, bool with_trj, bool with_parents, bool with_frames) {
    const int64_t lengths[] = {1, 2, 63, 64, 65, 257}, gap = 5;
    const int order[] = {3, 0, 5, 1, 4, 2};
    const int k = 6;
    int64_t first[6], total = gap;
    for (int i = 0; i < k; ++i) {
        first[order[i]] = total;
        total += lengths[order[i]] + gap;
    }
    uint32_t seed = 7u + (uint32_t)J;
    std::vector<float> pos((size_t)total * J * 3), gt((size_t)total * J * 3), trj((size_t)total * 3);
    for (auto &v : pos) v = rnd(seed);
    for (auto &v : gt) v = rnd(seed) + 2.0f;
    for (auto &v : trj) v = rnd(seed) + 2.0f;
    int32_t parents[17];
    for (int j = 0; j < 17; ++j) parents[j] = j - 1;
    const int32_t flags = with_trj ? R3D_VALID_POS_IS_SUM : R3D_VALID_GT_ROOT_RELATIVE;
    // valid clips with an invalid descriptor between any two
    const int64_t bad[][2] = {{5, 0}, {0, 258}, {total - 99, 100}, {-1, 50}, {INT64_MAX, 3}, {total, 1}};
    std::vector<r3d_clip_desc> table(2 * k);
    for (int c = 0; c < k; ++c) {
        std::memset(&table[2 * c], 0xff, 2 * sizeof(r3d_clip_desc));     // rn2w / tn2w: not read
        table[2 * c].first_frame = first[c];
        table[2 * c].n_frames = lengths[c];
        table[2 * c + 1].first_frame = bad[c][0];
        table[2 * c + 1].n_frames = bad[c][1];
    }
    const int64_t stride = R3D_VALID_DOUBLES + 3;
    std::vector<double> rows((size_t)(2 * k - 1) * stride + R3D_VALID_DOUBLES, -7.0), frame((size_t)total * R3D_VALID_COUNT, -7.0);
    const int rc = r3d_debug_clips_valid_losses_host(pos.data(), with_trj ? trj.data() : nullptr, gt.data(), total, J,
                                                     with_parents ? parents : nullptr, flags, table.data(), 2 * k, 257, rows.data(), stride,
                                                     with_frames ? frame.data() : nullptr);
    EXPECT(rc == 0);
    std::vector<bool> covered((size_t)total, false);
    for (int c = 0; c < k; ++c) {
        const int64_t n = lengths[c];
        std::vector<float> p(pos.begin() + first[c] * J * 3, pos.begin() + (first[c] + n) * J * 3);      // exact-size copies of the slice
        std::vector<float> g(gt.begin() + first[c] * J * 3, gt.begin() + (first[c] + n) * J * 3);
        std::vector<float> t(trj.begin() + first[c] * 3, trj.begin() + (first[c] + n) * 3);
        std::vector<double> want(R3D_VALID_DOUBLES), want_fr((size_t)n * R3D_VALID_COUNT);
        EXPECT(r3d_debug_valid_losses_host(p.data(), with_trj ? t.data() : nullptr, g.data(), n, J, with_parents ? parents : nullptr, flags,
                                           want.data(), want_fr.data()) == 0);
        EXPECT(same_bits(&rows[(size_t)(2 * c) * stride], want.data(), R3D_VALID_DOUBLES));
        if (with_frames) EXPECT(same_bits(&frame[(size_t)first[c] * R3D_VALID_COUNT], want_fr.data(), want_fr.size()));
        for (int64_t f = 0; f < n; ++f) covered[(size_t)(first[c] + f)] = true;
        const double *badrow = &rows[(size_t)(2 * c + 1) * stride];
        bool all_nan = true;
        for (int i = 0; i < R3D_VALID_DOUBLES; ++i) all_nan = all_nan && std::isnan(badrow[i]);
        EXPECT(all_nan);
        if (2 * c + 1 < 2 * k - 1)
            for (int i = R3D_VALID_DOUBLES; i < stride; ++i) EXPECT(badrow[i] == -7.0 && rows[(size_t)(2 * c) * stride + i] == -7.0);
    }
    for (int64_t f = 0; f < total; ++f)
        if (!covered[(size_t)f] || !with_frames)
            for (int i = 0; i < R3D_VALID_COUNT; ++i) EXPECT(frame[(size_t)f * R3D_VALID_COUNT + i] == -7.0);
    // the argument rules
    EXPECT(r3d_debug_clips_valid_losses_host(pos.data(), nullptr, gt.data(), total, J, nullptr, R3D_VALID_POS_IS_SUM, table.data(), 2 * k, 257,
                                             rows.data(), stride, nullptr) == R3D_ERR_ARG);
    EXPECT(r3d_debug_clips_valid_losses_host(pos.data(), nullptr, gt.data(), total, J, nullptr, 0, table.data(), 2 * k, 257, rows.data(),
                                             R3D_VALID_DOUBLES - 1, nullptr) == R3D_ERR_ARG);
    EXPECT(r3d_debug_clips_valid_losses_host(pos.data(), nullptr, gt.data(), total, J, nullptr, 0, table.data(), 0, 257, rows.data(), stride,
                                             nullptr) == R3D_ERR_ARG);
}

}  // namespace

int main() {
    for (int J : {1, 14, 17})
        for (int m = 0; m < 8; ++m) run(J, m & 1, m & 2, m & 4);
    if (failures) {
        std::fprintf(stderr, "%d expectation(s) failed\n", failures);
        return 1;
    }
    std::printf("san_clips_valid: ok\n");
    return 0;
}
