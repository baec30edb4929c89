// Stand-alone driver of r3d_debug_streams_step_host for `make san_streams_step` (ray3d_amd/csrc/Makefile): linked against
// libray3d_hip_san.so - the host objects built -fsanitize=address,undefined - and built with the same flags itself, it runs the
// argument checks, the head rule, the action step, the slot index and the point routines of r3d_streams_step on HOST memory only (no
// device call, no GPU needed).  Every buffer is an exact-size heap block (the sanitizer's red zones around it) whose first and last
// GUARD elements are a guard band of their own that must keep its fill: clips of 1 .. 40 frames side by side on a state nobody
// zeroed (RESTART, PUSH ..., DRAIN x lag, IDLE) against a restatement written here - edge padding at both ends, every frame once and
// in order, the mirrored copy -, centred and causal lags, two and three features, the pixel encodings, every refusal (unknown
// actions, PUSH after a drain, heads at the extremes of both fields, a full counter), and the argument rules.  Exit status 0: every
// result as expected and no sanitizer report.
#define R3D_TEST_HOOKS
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ray3d_hip.h"

namespace {

int failures = 0;

void expect(bool ok, const char *what, int line) {
    if (!ok) {
        std::fprintf(stderr, "san_streams_step.cpp:%d: %s\n", line, what);
        ++failures;
    }
}
#define EXPECT(c) expect((c), #c, __LINE__)

uint32_t next(uint32_t &s) {
    s = s * 1664525u + 1013904223u;
    return s;
}
float rnd(uint32_t &s) { return (float)((next(s) >> 8) & 0xffff) / 65536.0f - 0.5f; }

constexpr float FILL = -7.0f;
constexpr size_t GUARD = 64;

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
    int S, RF, lag, J, F, enc, width;
    Banded<int64_t> state;
    Banded<float> frame, x, xm;
    Banded<double> cam;
    Banded<int32_t> action, status;
    Banded<int64_t> emit;
    int32_t perm[17];
    Rig(int S_, int RF_, int lag_, int J_, int F_, int enc_)
        : S(S_), RF(RF_), lag(lag_), J(J_), F(F_), enc(enc_), width(enc_ == R3D_ENCODE_NONE ? F_ : 2),
          state((r3d_streams_state_bytes(S_, RF_, J_, F_) + 7) / 8, (int64_t)0xA5A5A5A5A5A5A5A5ull), frame((size_t)S_ * J_ * width, FILL),
          x((size_t)S_ * RF_ * J_ * F_, FILL), xm((size_t)S_ * RF_ * J_ * F_, FILL), cam((size_t)S_ * 16, 0.0), action(S_, 0), status(S_, -5),
          emit(S_, -99) {
        for (int j = 0; j < J; ++j) perm[j] = J - 1 - j;
        for (int s = 0; s < S; ++s) {       // {fx, fy, cx, cy, cos, sin, w, h, k1, k2, p1, p2, k3, 0, 0, 0}
            const double row[16] = {1100.0 + s, 1090.0, 510.0, 505.0 - s, 0.98, 0.2, 1000, 1002, -0.2, 0.24, -0.001, 0.002, -0.003, 0, 0, 0};
            std::memcpy(&cam[(size_t)s * 16], row, sizeof row);
        }
    }
    r3d_stream_head *heads() { return reinterpret_cast<r3d_stream_head *>(state.data()); }
    float *ring() { return reinterpret_cast<float *>(heads() + S); }
    int tick(bool mirror = true) {
        x.refill(), xm.refill(), status.refill(), emit.refill();
        const int rc = r3d_debug_streams_step_host(state.data(), S, RF, lag, J, F, enc, frame.data(), enc == R3D_ENCODE_NONE ? nullptr : cam.data(),
                                                   action.data(), x.data(), mirror ? xm.data() : nullptr, mirror ? perm : nullptr, emit.data(),
                                                   status.data());
        EXPECT(state.guards_clean() && frame.guards_clean() && x.guards_clean() && xm.guards_clean() && cam.guards_clean());
        EXPECT(action.guards_clean() && status.guards_clean() && emit.guards_clean());
        return rc;
    }
};

// clips of these lengths side by side against the restatement: row i of frame n's window is clip frame clamp(n - (RF-1-lag) + i, 0, N-1)
void run_clips(int J, int F, int RF, int lag) {
    const int lengths[] = {1, 2, 5, 13, 14, 40}, S = 6;
    Rig g(S, RF, lag, J, F, R3D_ENCODE_NONE);
    std::vector<std::vector<float>> clip(S);
    uint32_t seed = 5u + (uint32_t)J + 3u * (uint32_t)RF + (uint32_t)lag;
    for (int s = 0; s < S; ++s) {
        clip[s].resize((size_t)lengths[s] * J * F);
        for (float &v : clip[s]) v = rnd(seed);
    }
    const uint32_t payload = 0x7fc12345u;
    std::memcpy(&clip[3][(size_t)2 * J * F], &payload, 4);
    const size_t pt = (size_t)J * F;
    std::vector<int> emitted(S, 0);
    for (int t = 0; t < 40 + lag + 1; ++t) {
        for (size_t i = 0; i < g.frame.n; ++i) g.frame[i] = FILL + 2.0f;
        for (int s = 0; s < S; ++s) {
            const int n = lengths[s];
            g.action[s] = t < n ? (t == 0 ? R3D_STREAM_RESTART : R3D_STREAM_PUSH) : (t < n + lag ? R3D_STREAM_DRAIN : R3D_STREAM_IDLE);
            if (t < n) std::memcpy(&g.frame[(size_t)s * pt], &clip[s][(size_t)t * pt], pt * 4);
        }
        EXPECT(g.tick() == 0);
        for (int s = 0; s < S; ++s) {
            EXPECT(g.status[s] == 0);
            const int64_t n = g.emit[s];
            const int want = t - lag;                           // frame t - lag is complete at tick t
            if (want < 0 || want >= lengths[s]) {
                EXPECT(n == -1);
                EXPECT(bits(g.x[(size_t)s * RF * pt]) == bits(FILL) && bits(g.xm[(size_t)(s + 1) * RF * pt - 1]) == bits(FILL));
                continue;
            }
            EXPECT(n == want && n == emitted[s]);
            ++emitted[s];
            bool same = true;
            for (int i = 0; i < RF && same; ++i) {
                const int64_t f = std::min<int64_t>(std::max<int64_t>(n - (RF - 1 - lag) + i, 0), lengths[s] - 1);
                for (int j = 0; j < J && same; ++j)
                    for (int c = 0; c < F && same; ++c) {
                        const size_t at = ((size_t)(s * RF + i) * J + j) * F + c;
                        same = bits(g.x[at]) == bits(clip[s][((size_t)f * J + j) * F + c]) &&
                               bits(g.xm[at]) == (bits(clip[s][((size_t)f * J + g.perm[j]) * F + c]) ^ (c == 0 ? 0x80000000u : 0u));
                    }
            }
            EXPECT(same);
        }
    }
    for (int s = 0; s < S; ++s) EXPECT(emitted[s] == lengths[s] && g.heads()[s].count == lengths[s] && g.heads()[s].drained == lag);
}

// every refusal: status 1, emit -1, nothing of the stream written; the neighbour goes on
void run_refusals(int RF, int lag) {
    const int J = 14, F = 2, S = 2;
    Rig g(S, RF, lag, J, F, R3D_ENCODE_NONE);
    uint32_t seed = 77u;
    auto fresh = [&] { for (size_t i = 0; i < g.frame.n; ++i) g.frame[i] = rnd(seed); };
    for (int t = 0; t < 5; ++t) {
        fresh();
        g.action[0] = g.action[1] = t == 0 ? R3D_STREAM_RESTART : R3D_STREAM_PUSH;
        EXPECT(g.tick() == 0 && g.status[0] == 0 && g.status[1] == 0);
    }
    const int64_t big = INT64_MAX, small = INT64_MIN, full = (int64_t)1 << 62;
    struct Case { int64_t count, drained; int32_t action; } cases[] = {
        {5, 0, 4}, {5, 0, -1}, {5, 0, INT32_MAX}, {5, 0, INT32_MIN}, {-1, 0, R3D_STREAM_PUSH}, {-1, 0, R3D_STREAM_DRAIN}, {small, 0, R3D_STREAM_PUSH},
        {big, 0, R3D_STREAM_DRAIN}, {full + 1, 0, R3D_STREAM_PUSH}, {full, 0, R3D_STREAM_PUSH}, {5, lag + 1, R3D_STREAM_PUSH}, {5, lag + 1, R3D_STREAM_DRAIN},
        {5, -1, R3D_STREAM_PUSH}, {5, big, R3D_STREAM_DRAIN}, {5, small, R3D_STREAM_DRAIN}, {big, big, R3D_STREAM_PUSH}};
    for (const Case &c : cases) {
        g.heads()[0].count = c.count;
        g.heads()[0].drained = c.drained;
        std::vector<int64_t> before(g.state.mem);
        const int64_t count1 = g.heads()[1].count;
        fresh();
        g.action[0] = c.action;
        g.action[1] = R3D_STREAM_PUSH;
        EXPECT(g.tick() == 0);
        EXPECT(g.status[0] == 1 && g.emit[0] == -1 && g.status[1] == 0 && g.heads()[1].count == count1 + 1);
        EXPECT(bits(g.x[0]) == bits(FILL) && bits(g.xm[(size_t)RF * J * F - 1]) == bits(FILL));
        const size_t ring_words = (size_t)RF * J * F * 4 / 8;     // ring 0 sits behind the S heads (RF * J * F is even here)
        EXPECT(!std::memcmp(g.heads(), before.data() + GUARD, 16));
        EXPECT(!std::memcmp(g.state.data() + 2 * S, before.data() + GUARD + 2 * S, ring_words * 8));
    }
    // the last count a stream can reach; PUSH after a drain began; RESTART afterwards
    g.heads()[0].count = full - 1;
    g.heads()[0].drained = 0;
    fresh();
    g.action[0] = R3D_STREAM_PUSH;
    g.action[1] = R3D_STREAM_IDLE;
    EXPECT(g.tick() == 0 && g.status[0] == 0 && g.emit[0] == full - 1 - lag && g.heads()[0].count == full);
    g.action[0] = R3D_STREAM_DRAIN;
    EXPECT(g.tick() == 0 && g.status[0] == 0 && (lag ? g.emit[0] == full - lag && g.heads()[0].drained == 1 : g.emit[0] == -1));
    g.action[0] = R3D_STREAM_PUSH;
    EXPECT(g.tick() == 0 && g.status[0] == 1);                   // (lag 0: the counter is full; otherwise the drain began)
    g.action[0] = R3D_STREAM_RESTART;
    EXPECT(g.tick() == 0 && g.status[0] == 0 && g.heads()[0].count == 1 && g.heads()[0].drained == 0 && g.emit[0] == (lag ? -1 : 0));
    EXPECT(g.status[1] == 0 && g.emit[1] == -1);
}

// the pixel encodings: finite values arrive, NaN pixels leave as the canonical quiet NaN, nothing outside the extents
void run_pixels(int enc, int RF, int lag) {
    const int J = 17, S = 3, F = enc == R3D_ENCODE_RAY ? 3 : 2;
    Rig g(S, RF, lag, J, F, enc);
    uint32_t seed = 9u + (uint32_t)enc;
    for (int t = 0; t < RF + 3; ++t) {
        for (size_t i = 0; i < g.frame.n; ++i) g.frame[i] = 500.0f + 900.0f * rnd(seed);
        if (t == 2) g.frame[5] = __builtin_nanf("0x123");
        for (int s = 0; s < S; ++s) g.action[s] = t == 0 ? R3D_STREAM_RESTART : R3D_STREAM_PUSH;
        EXPECT(g.tick(t & 1) == 0);
        for (int s = 0; s < S; ++s) EXPECT(g.status[s] == 0 && g.emit[s] == (t - lag < 0 ? -1 : t - lag));
    }
    bool finite = true;
    for (size_t i = 0; i < g.x.n; ++i) finite = finite && g.x[i] == g.x[i];
    EXPECT(finite);                                              // (frame 2 has left every window by now)
}

void run_arguments() {
    Rig g(3, 9, 4, 17, 3, R3D_ENCODE_NONE);
    auto call = [&](void *state, int S, int RF, int lag, int J, int F, int enc, const float *frame, const double *cam, const int32_t *action, float *x,
                    float *xm, const int32_t *perm, int64_t *emit, int32_t *status) {
        return r3d_debug_streams_step_host(state, S, RF, lag, J, F, enc, frame, cam, action, x, xm, perm, emit, status);
    };
    void *st = g.state.data();
    float *fr = g.frame.data(), *x = g.x.data(), *xm = g.xm.data();
    double *cam = g.cam.data();
    int32_t *ac = g.action.data(), *ss = g.status.data(), *pm = g.perm;
    int64_t *em = g.emit.data();
    int32_t twice[17] = {0}, out_of_range[17];
    for (int j = 0; j < 17; ++j) out_of_range[j] = j;
    out_of_range[3] = 17;
    const int N = R3D_ENCODE_NONE, E = R3D_ERR_ARG;
    EXPECT(call(nullptr, 3, 9, 4, 17, 3, N, fr, cam, ac, x, xm, pm, em, ss) == E);
    EXPECT(call(st, 3, 9, 4, 17, 3, N, nullptr, cam, ac, x, xm, pm, em, ss) == E);
    EXPECT(call(st, 3, 9, 4, 17, 3, N, fr, cam, nullptr, x, xm, pm, em, ss) == E);
    EXPECT(call(st, 3, 9, 4, 17, 3, N, fr, cam, ac, nullptr, xm, pm, em, ss) == E);
    EXPECT(call(st, 3, 9, 4, 17, 3, N, fr, cam, ac, x, xm, pm, nullptr, ss) == E);
    EXPECT(call(st, 3, 9, 4, 17, 3, N, fr, cam, ac, x, xm, pm, em, nullptr) == E);
    EXPECT(call(st, 0, 9, 4, 17, 3, N, fr, cam, ac, x, xm, pm, em, ss) == E);
    EXPECT(call(st, R3D_CLIPS_MAX + 1, 9, 4, 17, 3, N, fr, cam, ac, x, xm, pm, em, ss) == E);
    EXPECT(call(st, 3, 9, 4, 0, 3, N, fr, cam, ac, x, nullptr, nullptr, em, ss) == E);
    EXPECT(call(st, 3, 9, 4, 18, 3, N, fr, cam, ac, x, nullptr, nullptr, em, ss) == E);
    EXPECT(call(st, 3, 0, 0, 17, 3, N, fr, cam, ac, x, xm, pm, em, ss) == E);
    EXPECT(call(st, 3, 9, -1, 17, 3, N, fr, cam, ac, x, xm, pm, em, ss) == E);
    EXPECT(call(st, 3, 9, 9, 17, 3, N, fr, cam, ac, x, xm, pm, em, ss) == E);
    EXPECT(call(st, 3, 9, 4, 17, 3, 4, fr, cam, ac, x, xm, pm, em, ss) == E);
    EXPECT(call(st, 3, 9, 4, 17, 3, -1, fr, cam, ac, x, xm, pm, em, ss) == E);
    EXPECT(call(st, 3, 9, 4, 17, 1, N, fr, cam, ac, x, xm, pm, em, ss) == E);
    EXPECT(call(st, 3, 9, 4, 17, 4, N, fr, cam, ac, x, xm, pm, em, ss) == E);
    EXPECT(call(st, 3, 9, 4, 17, 2, R3D_ENCODE_RAY, fr, cam, ac, x, xm, pm, em, ss) == E);
    EXPECT(call(st, 3, 9, 4, 17, 3, R3D_ENCODE_INTRINSIC, fr, cam, ac, x, xm, pm, em, ss) == E);
    EXPECT(call(st, 3, 9, 4, 17, 3, R3D_ENCODE_SCREEN, fr, cam, ac, x, xm, pm, em, ss) == E);
    EXPECT(call(st, 3, 9, 4, 17, 3, R3D_ENCODE_RAY, fr, nullptr, ac, x, xm, pm, em, ss) == E);
    EXPECT(call(st, 3, 9, 4, 17, 3, N, fr, cam, ac, x, nullptr, pm, em, ss) == E);
    EXPECT(call(st, 3, 9, 4, 17, 3, N, fr, cam, ac, x, xm, nullptr, em, ss) == E);
    EXPECT(call(st, 3, 9, 4, 17, 3, N, fr, cam, ac, x, xm, twice, em, ss) == E);
    EXPECT(call(st, 3, 9, 4, 17, 3, N, fr, cam, ac, x, xm, out_of_range, em, ss) == E);
    EXPECT(call(st, 1, R3D_ENCODE_MAX_POINTS / 17 + 1, 0, 17, 3, N, fr, cam, ac, x, xm, pm, em, ss) == E);
    EXPECT(call(st, 200, 1 << 20, 0, 17, 3, N, fr, cam, ac, x, xm, pm, em, ss) == E);
    EXPECT(call(reinterpret_cast<char *>(st) + 4, 3, 9, 4, 17, 3, N, fr, cam, ac, x, xm, pm, em, ss) == E);
    EXPECT(call(st, 3, 9, 4, 17, 3, N, fr, cam, ac, x, xm, pm, reinterpret_cast<int64_t *>(reinterpret_cast<char *>(em) + 4), ss) == E);
    EXPECT(r3d_last_error()[0] != 0);
    for (size_t i = 0; i < g.x.n; ++i) EXPECT(bits(g.x[i]) == bits(FILL));          // nothing was written
    EXPECT(g.heads()[0].count == (int64_t)0xA5A5A5A5A5A5A5A5ull);
    EXPECT(r3d_streams_state_bytes(3, 9, 17, 3) == 3 * 16 + 3 * 9 * 17 * 3 * 4 && r3d_streams_state_bytes(0, 9, 17, 3) == 0);
    EXPECT(r3d_streams_state_bytes(3, 9, 17, 4) == 0 && r3d_streams_state_bytes(200, 1 << 20, 17, 3) == 0);
    EXPECT(sizeof(r3d_stream_head) == 16);
}

}  // namespace

int main() {
    for (int lag : {13, 0}) run_clips(17, 3, 27, lag);
    for (int lag : {4, 0, 8}) run_clips(14, 2, 9, lag);
    run_clips(1, 2, 1, 0);
    run_refusals(9, 4);
    run_refusals(9, 0);
    run_pixels(R3D_ENCODE_RAY, 27, 13);
    run_pixels(R3D_ENCODE_INTRINSIC, 9, 0);
    run_pixels(R3D_ENCODE_SCREEN, 9, 4);
    run_arguments();
    if (failures) {
        std::fprintf(stderr, "san_streams_step: %d expectation(s) failed\n", failures);
        return 1;
    }
    std::puts("san_streams_step: ok");
    return 0;
}
