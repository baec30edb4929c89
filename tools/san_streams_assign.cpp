// Stand-alone driver of r3d_debug_streams_assign_host for `make san_streams_assign` (ray3d_amd/csrc/Makefile): linked against
// libray3d_hip_san.so - the host objects built -fsanitize=address,undefined - and built with the same flags itself, it runs the
// argument checks, the state's layout, the per-detection, per-pair and per-slot routines and the greedy matching of
// r3d_streams_assign on HOST memory only (no device call, no GPU needed).  Every buffer is an exact-size heap block (the sanitizer's
// red zones around it) whose first and last GUARD elements are a guard band of their own that must keep its fill.  It plays seeded
// ticks - people who enter, walk, lose joints and detections and leave, det_count below 0 and above D, non-finite keypoints and
// confidences, a state of 0xA5 bytes - over the extreme shapes (1 x 1, 32 x 1, 1 x 32, 32 x 32 slots x detections), both widths, both
// fills, lags 0, 1 and 4, and checks what must hold whatever the inputs are: every output element written, a match names a
// detection below the clamped count and no detection twice, a pushed row is that detection's bits, identities are unique per
// camera and never reused, the stats add up; then every refusal of the argument rules.  Exit status 0: every result as expected
// and no sanitizer report.
#define R3D_TEST_HOOKS
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <set>
#include <vector>

#include "ray3d_hip.h"

namespace {

int failures = 0;

void expect(bool ok, const char *what, int line) {
    if (!ok) {
        std::fprintf(stderr, "san_streams_assign.cpp:%d: %s\n", line, what);
        ++failures;
    }
}
#define EXPECT(c) expect((c), #c, __LINE__)

uint32_t next(uint32_t &s) {
    s = s * 1664525u + 1013904223u;
    return s;
}
float rnd(uint32_t &s) { return (float)((next(s) >> 8) & 0xffff) / 65536.0f; }      // [0, 1)

constexpr size_t GUARD = 64;
constexpr int32_t POISON = (int32_t)0xA5A5A5A5;

// an exact-size heap block: GUARD elements of fill, the payload, GUARD elements of fill
template <class T> struct Banded {
    std::vector<T> mem;
    size_t n;
    T fill;
    Banded(size_t count, T f) : mem(count + 2 * GUARD, f), n(count), fill(f) {}
    T *data() { return mem.data() + GUARD; }
    T &operator[](size_t i) { return mem[GUARD + i]; }
    void refill() { std::fill(mem.begin() + GUARD, mem.begin() + GUARD + n, fill); }
    bool guards_clean() const {
        for (size_t i = 0; i < GUARD; ++i)
            if (std::memcmp(&mem[i], &fill, sizeof(T)) || std::memcmp(&mem[GUARD + n + i], &fill, sizeof(T))) return false;
        return true;
    }
};

uint32_t bits(float v) {
    uint32_t b;
    std::memcpy(&b, &v, 4);
    return b;
}

// the buffers of one caller; the state is int64 words so that the heap block is 8-byte aligned
struct Rig {
    r3d_assign_params prm;
    int S;
    Banded<int64_t> state, id;
    Banded<float> det, conf, frame_out, conf_out;
    Banded<int32_t> count, action, match, stats;
    Rig(int C, int P, int D, int J, int width, int lag, int fill, bool poisoned)
        : prm{(int32_t)sizeof(r3d_assign_params), C, P, D, J, width, lag, std::min(4, J), std::min(3, J), 2, fill, 0.3f, 0.5},
          S(C * P), state(r3d_streams_assign_bytes(C, P, J, width) / 8, poisoned ? (int64_t)0xA5A5A5A5A5A5A5A5ull : 0), id(S, -77),
          det((size_t)C * D * J * width, 0.0f), conf((size_t)C * D * J, 1.0f), frame_out((size_t)S * J * width, -7.0f),
          conf_out((size_t)S * J, -7.0f), count(C, 0), action(S, POISON), match(S, POISON), stats((size_t)C * 4, POISON) {}
    int run(bool with_conf = true) {
        return r3d_debug_streams_assign_host(state.data(), &prm, det.data(), with_conf ? conf.data() : nullptr, count.data(), action.data(),
                                             frame_out.data(), conf_out.data(), match.data(), id.data(), stats.data());
    }
    bool guards_clean() const {
        return state.guards_clean() && id.guards_clean() && det.guards_clean() && conf.guards_clean() && frame_out.guards_clean() &&
               conf_out.guards_clean() && count.guards_clean() && action.guards_clean() && match.guards_clean() && stats.guards_clean();
    }
};

// seeded ticks on one shape, with the invariants that hold whatever the inputs are
void play(int C, int P, int D, int J, int width, int lag, int fill, bool poisoned, bool with_conf, uint32_t seed) {
    Rig r(C, P, D, J, width, lag, fill, poisoned);
    const int people = std::min(std::max(P, D) + 2, 10), ticks = lag + 2 + 3 + 8;
    std::vector<std::set<int64_t>> known(C);           // identities seen per camera ...
    std::vector<int64_t> owner(r.S, -1);               // ... and the one a slot held on the previous tick
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (int t = 0; t < ticks; ++t) {
        for (int c = 0; c < C; ++c) {
            int n = 0;
            for (int k = 0; k < people && n < D; ++k) {
                if ((t + k) % 7 >= 5 || rnd(seed) < 0.2f) continue;         // away, or not detected
                float *row = &r.det[((size_t)c * D + n) * J * width];
                for (int j = 0; j < J; ++j) {
                    const bool gone = rnd(seed) < 0.25f;
                    row[j * width] = gone ? nan : 260.0f * k + 8.0f * t + 200.0f * ((j * 37) % 17) / 16.0f + 2.0f * rnd(seed);
                    row[j * width + 1] = gone ? nan : 100.0f + 200.0f * ((j * 23) % 17) / 16.0f + 2.0f * rnd(seed);
                    if (width == 3) row[j * width + 2] = 1.0f;
                    r.conf[((size_t)c * D + n) * J + j] = 0.2f + rnd(seed);
                }
                ++n;
            }
            for (int d = n; d < D; ++d)                                      // rows behind the count: never read below it
                for (int i = 0; i < J * width; ++i) r.det[((size_t)c * D + d) * J * width + i] = 5000.0f + 300.0f * d + (float)(i % 7);
            r.count[c] = n;
            if (t == 2) r.count[c] = -3;
            if (t == 3) r.count[c] = D + 7;
            if (t == 4 && n >= 1) {
                r.det[(size_t)c * D * J * width] = inf;
                r.det[(size_t)c * D * J * width + width + 1] = -inf;
                r.conf[(size_t)c * D * J + 2 % J] = nan;
            }
        }
        r.frame_out.refill(), r.conf_out.refill(), r.action.refill(), r.match.refill(), r.stats.refill(), r.id.refill();
        EXPECT(r.run(with_conf) == 0);
        EXPECT(r.guards_clean());
        for (int c = 0; c < C; ++c) {
            const int n = std::min(std::max(r.count[c], 0), D);
            std::set<int> used;
            int matched = 0, born = 0;
            for (int p = 0; p < P; ++p) {
                const int s = c * P + p, a = r.action[s], m = r.match[s];
                EXPECT(a >= R3D_STREAM_IDLE && a <= R3D_STREAM_DRAIN);
                EXPECT(m >= -1 && m < n);
                EXPECT(lag > 0 || a != R3D_STREAM_DRAIN);
                const bool pushes = a == R3D_STREAM_PUSH || a == R3D_STREAM_RESTART;
                if (m >= 0) {
                    EXPECT(pushes && used.insert(m).second);
                    EXPECT(!std::memcmp(&r.frame_out[(size_t)s * J * width], &r.det[((size_t)c * D + m) * J * width], sizeof(float) * J * width));
                    matched += a == R3D_STREAM_PUSH;
                    born += a == R3D_STREAM_RESTART;
                } else {
                    EXPECT(a != R3D_STREAM_RESTART);
                }
                for (int i = 0; i < J * width; ++i) {
                    const uint32_t b = bits(r.frame_out[(size_t)s * J * width + i]);
                    EXPECT(b != bits(-7.0f));                                 // written
                    if (m < 0 && !(a == R3D_STREAM_PUSH && fill == R3D_ASSIGN_FILL_HOLD)) EXPECT(b == 0x7fc00000u);
                }
                for (int j = 0; j < J; ++j) {
                    const uint32_t b = bits(r.conf_out[(size_t)s * J + j]);
                    EXPECT(m >= 0 ? b == (with_conf ? bits(r.conf[((size_t)c * D + m) * J + j]) : 0x3f800000u) : b == 0u);
                }
                const int64_t id = r.id[s];
                if (a == R3D_STREAM_RESTART) EXPECT(known[c].insert(id).second);            // a new identity, never a used one
                else if (!(a == R3D_STREAM_IDLE && id == -1)) EXPECT(id == owner[s]);      // a live or draining slot keeps its own
                owner[s] = a == R3D_STREAM_IDLE ? -1 : id;
            }
            const int32_t *st = &r.stats[(size_t)c * 4];
            EXPECT(st[1] == matched && st[2] == born && st[0] >= st[1] + st[2] && st[3] == st[0] - st[1] - st[2] && st[0] <= n);
        }
    }
}

void argument_rules() {
    Rig r(2, 3, 5, 17, 3, 4, R3D_ASSIGN_FILL_NAN, false);
    for (int c = 0; c < 2; ++c) r.count[c] = 0;
    EXPECT(r.run() == 0);
    const r3d_assign_params good = r.prm;
    auto refused = [&](const r3d_assign_params &p) {
        r.prm = p;
        const int rc = r.run();
        r.prm = good;
        return rc == R3D_ERR_ARG && r3d_last_error()[0] != 0;
    };
    r3d_assign_params p = good;
    p.struct_size = 0; EXPECT(refused(p)); p = good;
    p.struct_size += 8; EXPECT(refused(p)); p = good;
    p.num_cameras = 0; EXPECT(refused(p)); p = good;
    p.slots = 0; EXPECT(refused(p)); p = good;
    p.slots = R3D_ASSIGN_MAX_SLOTS + 1; EXPECT(refused(p)); p = good;
    p.max_detections = 0; EXPECT(refused(p)); p = good;
    p.max_detections = R3D_ASSIGN_MAX_DETECTIONS + 1; EXPECT(refused(p)); p = good;
    p.num_cameras = R3D_CLIPS_MAX / 3 + 1; EXPECT(refused(p)); p = good;
    p.num_joints = 0; EXPECT(refused(p)); p = good;
    p.num_joints = 18; EXPECT(refused(p)); p = good;
    p.width = 1; EXPECT(refused(p)); p = good;
    p.width = 4; EXPECT(refused(p)); p = good;
    p.lag = -1; EXPECT(refused(p)); p = good;
    p.min_joints = 0; EXPECT(refused(p)); p = good;
    p.min_joints = 18; EXPECT(refused(p)); p = good;
    p.min_common = 0; EXPECT(refused(p)); p = good;
    p.min_common = 18; EXPECT(refused(p)); p = good;
    p.max_missed = -1; EXPECT(refused(p)); p = good;
    p.fill = 2; EXPECT(refused(p)); p = good;
    p.min_conf = std::numeric_limits<float>::quiet_NaN(); EXPECT(refused(p)); p = good;
    p.min_conf = std::numeric_limits<float>::infinity(); EXPECT(refused(p)); p = good;
    p.max_cost = 0.0; EXPECT(refused(p)); p = good;
    p.max_cost = std::numeric_limits<double>::quiet_NaN(); EXPECT(refused(p)); p = good;
    p.max_cost = std::numeric_limits<double>::infinity(); EXPECT(refused(p)); p = good;
    void *state = r.state.data();
    float *det = r.det.data(), *conf = r.conf.data(), *fo = r.frame_out.data(), *co = r.conf_out.data();
    int32_t *count = r.count.data(), *action = r.action.data(), *match = r.match.data(), *stats = r.stats.data();
    int64_t *id = r.id.data();
    auto call = [&](void *a_state, const r3d_assign_params *a_prm, const float *a_det, const int32_t *a_count, int32_t *a_action, float *a_fo,
                    float *a_co, int32_t *a_match, int64_t *a_id, int32_t *a_stats) {
        return r3d_debug_streams_assign_host(a_state, a_prm, a_det, conf, a_count, a_action, a_fo, a_co, a_match, a_id, a_stats);
    };
    EXPECT(call(nullptr, &good, det, count, action, fo, co, match, id, stats) == R3D_ERR_ARG);
    EXPECT(call(state, nullptr, det, count, action, fo, co, match, id, stats) == R3D_ERR_ARG);
    EXPECT(call(state, &good, nullptr, count, action, fo, co, match, id, stats) == R3D_ERR_ARG);
    EXPECT(call(state, &good, det, nullptr, action, fo, co, match, id, stats) == R3D_ERR_ARG);
    EXPECT(call(state, &good, det, count, nullptr, fo, co, match, id, stats) == R3D_ERR_ARG);
    EXPECT(call(state, &good, det, count, action, nullptr, co, match, id, stats) == R3D_ERR_ARG);
    EXPECT(call(state, &good, det, count, action, fo, co, nullptr, id, stats) == R3D_ERR_ARG);
    EXPECT(call(state, &good, det, count, action, fo, co, match, nullptr, stats) == R3D_ERR_ARG);
    // alignment, and an output over an input, the state and another output
    EXPECT(call(static_cast<char *>(state) + 4, &good, det, count, action, fo, co, match, id, stats) == R3D_ERR_ARG);
    EXPECT(call(state, &good, det, count, action, fo, co, match, reinterpret_cast<int64_t *>(reinterpret_cast<char *>(id) + 4), stats) == R3D_ERR_ARG);
    EXPECT(call(state, &good, det, count, reinterpret_cast<int32_t *>(det), fo, co, match, id, stats) == R3D_ERR_ARG);
    EXPECT(call(state, &good, det, count, action, fo, co, match, id, count) == R3D_ERR_ARG);
    EXPECT(call(state, &good, det, count, action, static_cast<float *>(state), co, match, id, stats) == R3D_ERR_ARG);
    EXPECT(call(state, &good, det, count, action, fo, co, action + 5, id, stats) == R3D_ERR_ARG);
    EXPECT(call(state, &good, det, count, action, fo, fo + 6 * 17 * 3 - 1, match, id, stats) == R3D_ERR_ARG);
    // what is optional
    EXPECT(call(state, &good, det, count, action, fo, nullptr, match, id, nullptr) == 0);
    EXPECT(r.guards_clean());
    EXPECT(r3d_streams_assign_bytes(2, 3, 17, 3) == (size_t)(8 * 2 + 6 * (8 + 16 + 4 * 17 * 3)));
    EXPECT(r3d_streams_assign_bytes(1, 33, 17, 3) == 0 && r3d_streams_assign_bytes(1, 1, 17, 4) == 0 && r3d_streams_assign_bytes(0, 1, 17, 2) == 0);
}

}  // namespace

int main() {
    const int shapes[6][3] = {{1, 1, 1}, {2, 3, 5}, {3, 5, 3}, {2, 32, 1}, {2, 1, 32}, {1, 32, 32}};
    const int lags[3] = {0, 1, 4};
    int k = 0;
    for (const auto &sh : shapes)
        for (int J : {14, 17})
            for (int width : {2, 3}) {
                play(sh[0], sh[1], sh[2], J, width, lags[k % 3], (k / 2) % 2, k % 4 == 2, k % 2 == 1, 1234u + 17u * k);
                ++k;
            }
    argument_rules();
    if (failures) {
        std::fprintf(stderr, "san_streams_assign: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("san_streams_assign: ok (%d cases)\n", k);
    return 0;
}
