// Stand-alone driver of r3d_debug_clips_windows_host for `make san_clips_windows` (ray3d_amd/csrc/Makefile): linked against
// libray3d_hip_san.so - the host objects built -fsanitize=address,undefined - and built with the same flags itself, it runs the
// argument checks, the bisection, the descriptor rule and the per-point routine of r3d_clips_windows on HOST memory only (no device
// call, no GPU needed).  Every buffer is an exact-size heap block (the sanitizer's red zones around it) whose first and last GUARD
// elements are a guard band of their own that must keep its fill: evaluation clips of 1 .. 100 frames pooled and lifted in batches
// that cut them, centred and causal starts, steps above one, flip runs, clips out of order with gaps in the source, clips that end
// on the last source row, surplus windows, every kind of invalid descriptor (the extremes of every field included), shuffled,
// overlapping and random tables, and the argument rules.  Exit status 0: every result as expected and no sanitizer report.
#define R3D_TEST_HOOKS
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ray3d_hip.h"

namespace {

int failures = 0;

void expect(bool ok, const char *what, int line) {
    if (!ok) {
        std::fprintf(stderr, "san_clips_windows.cpp:%d: %s\n", line, what);
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

bool valid(const r3d_window_run_desc &d, int64_t total, bool has_perm) {
    const __int128 lim = R3D_ENCODE_MAX_POINTS;
    if (d.n_frames < 1 || d.n_windows < 1 || d.step < 1 || (d.flip != 0 && d.flip != 1) || (d.flip && !has_perm)) return false;
    if (d.first_frame < 0 || (__int128)d.first_frame + d.n_frames > total || d.win_first < 0 || d.n_windows > lim) return false;
    if (d.start < -lim || d.start > lim) return false;
    return (__int128)d.start + (__int128)(d.n_windows - 1) * d.step <= lim;
}

void run(int J, int F, int RF, bool causal, bool with_param, bool with_perm) {
    const int64_t lengths[] = {1, 2, 5, 13, 14, 40, 100}, gap = 2;
    const int order[] = {4, 0, 6, 2, 5, 1, 3}, nclip = 7, E = 2;
    int64_t first[7], total = 0;
    for (int i = 0; i < nclip; ++i) {                            // no gap in front and none behind: clips touch both ends
        first[order[i]] = total;
        total += lengths[order[i]] + (i + 1 < nclip ? gap : 0);
    }
    uint32_t seed = 11u + (uint32_t)J * 7u + (uint32_t)RF;
    Banded<float> src((size_t)total * J * F, FILL + 1.0f);
    for (size_t i = 0; i < src.n; ++i) src[i] = rnd(seed);
    const uint32_t payload = 0x7fc12345u;
    std::memcpy(&src[(size_t)(first[3] + 2) * J * F], &payload, 4);
    int32_t perm[17];
    for (int j = 0; j < J; ++j) perm[j] = J - 1 - j;
    const int pad = (RF - 1) / 2;
    // the valid runs: every clip once (step 1, evaluation windows), then three more over the same frames: steps 2 and 3, flips
    std::vector<r3d_window_run_desc> good;
    int64_t at = 0;
    for (int c = 0; c < nclip + 3; ++c) {
        const int clip = c < nclip ? c : (c - nclip) * 2 + 2;
        r3d_window_run_desc d;
        d.first_frame = first[clip];
        d.n_frames = lengths[clip];
        d.win_first = at;
        d.n_windows = c < nclip ? lengths[clip] : 4 + c;
        d.start = -(int64_t)(pad + (causal ? pad : 0)) - (c < nclip ? 0 : c);
        d.step = c < nclip ? 1 : c - nclip + 2;
        d.flip = with_perm ? c & 1 : 0;
        at += d.n_windows;
        good.push_back(d);
    }
    good.back().n_windows += 9;                                  // the surplus of the last batch
    at += 9;
    const int64_t windows = at, big = INT64_MAX, small = INT64_MIN;
    // invalid runs: {first_frame, n_frames, n_windows, start, step, flip} in place of run `r` (its window slots kept)
    const int64_t lim = R3D_ENCODE_MAX_POINTS;
    const int64_t bad[][6] = {{0, 0, 3, 0, 1, 0},       {0, -1, 3, 0, 1, 0},      {0, 1, 0, 0, 1, 0},      {0, 1, -5, 0, 1, 0},      {0, 1, 3, 0, 0, 0},
                              {0, 1, 3, 0, -1, 0},      {0, 1, 3, 0, 1, 2},       {0, 1, 3, 0, 1, -1},     {-1, 1, 3, 0, 1, 0},      {total, 1, 3, 0, 1, 0},
                              {total - 4, 5, 3, 0, 1, 0}, {0, total + 1, 3, 0, 1, 0}, {big, 1, 3, 0, 1, 0},  {0, big, 3, 0, 1, 0},     {small, big, 3, 0, 1, 0},
                              {0, 1, 3, lim + 1, 1, 0}, {0, 1, 3, -lim - 1, 1, 0}, {0, 1, 3, big, 1, 0},    {0, 1, 3, small, 1, 0},   {0, 1, lim + 1, 0, 1, 0},
                              {0, 1, big, 0, 1, 0},     {0, 1, lim, 0, 2, 0},     {0, 1, lim, lim, INT32_MAX, 0}, {0, 1, 3, 0, INT32_MIN, 0}, {0, 1, 2, lim, 1, 0}};
    const int nbad = (int)(sizeof(bad) / sizeof(bad[0]));
    for (int variant = -1; variant < nbad + 1; ++variant) {       // -1: the valid table; nbad: a flip run without mirror_perm (if none is given)
        std::vector<r3d_window_run_desc> table = good;
        const int r = 3 + (variant + 1) % 5;
        if (variant >= 0 && variant < nbad) {
            table[(size_t)r].first_frame = bad[variant][0];
            table[(size_t)r].n_frames = bad[variant][1];
            table[(size_t)r].n_windows = bad[variant][2];
            table[(size_t)r].start = bad[variant][3];
            table[(size_t)r].step = (int32_t)bad[variant][4];
            table[(size_t)r].flip = (int32_t)bad[variant][5];
        } else if (variant == nbad) {
            table[(size_t)r].flip = 1;
        }
        const int nr = (int)table.size();
        Banded<r3d_window_run_desc> tab((size_t)nr, good[0]);
        for (int i = 0; i < nr; ++i) tab[(size_t)i] = table[(size_t)i];
        Banded<float> rp((size_t)nr * E, FILL);
        for (size_t i = 0; i < rp.n; ++i) rp[i] = rnd(seed);
        const int64_t batch = 32;
        for (int64_t w0 = 0; w0 < windows + batch; w0 += batch) {  // the last launch lies past every run
            Banded<float> x((size_t)batch * RF * J * F, FILL), param((size_t)batch * E, FILL);
            Banded<int32_t> status((size_t)nr, -1);
            const int rc = r3d_debug_clips_windows_host(src.data(), total, J, F, RF, tab.data(), nr, with_param ? rp.data() : nullptr, with_param ? E : 0,
                                                        w0, batch, x.data(), with_param ? param.data() : nullptr, with_perm ? perm : nullptr, status.data());
            EXPECT(rc == 0);
            EXPECT(src.guards_clean() && rp.guards_clean() && x.guards_clean() && param.guards_clean() && status.guards_clean());
            std::vector<int32_t> want((size_t)nr, -1);
            for (int64_t w = 0; w < batch; ++w) {
                const int64_t g = w0 + w;
                int run_of = 0;
                for (int i = 0; i < nr; ++i)
                    if (good[(size_t)i].win_first <= g) run_of = i;   // (win_first is never edited: the table stays sorted)
                const r3d_window_run_desc &d = table[(size_t)run_of];
                const bool ok = valid(d, total, with_perm);
                const bool member = ok && g - d.win_first < d.n_windows;
                if (!ok) want[(size_t)run_of] = 1;
                else if (member) want[(size_t)run_of] = 0;
                for (int i = 0; i < RF; ++i)
                    for (int j = 0; j < J; ++j)
                        for (int f = 0; f < F; ++f) {
                            const float got = x[(size_t)(((w * RF + i) * J + j) * F + f)];
                            if (!member) {
                                EXPECT(got == FILL);
                                continue;
                            }
                            __int128 t = (__int128)d.start + (__int128)(g - d.win_first) * d.step + i;
                            t = t < 0 ? 0 : (t > d.n_frames - 1 ? d.n_frames - 1 : t);
                            const int sj = d.flip ? perm[j] : j;
                            const uint32_t s = bits(src[(size_t)(((d.first_frame + (int64_t)t) * J + sj) * F + f)]);
                            EXPECT(bits(got) == (d.flip && f == 0 ? s ^ 0x80000000u : s));
                        }
                for (int e = 0; e < E; ++e) {
                    const float got = param[(size_t)(w * E + e)];
                    EXPECT(member && with_param ? bits(got) == bits(rp[(size_t)(run_of * E + e)]) : got == FILL);
                }
            }
            for (int i = 0; i < nr; ++i) EXPECT(status[(size_t)i] == want[(size_t)i]);
        }
    }
    // garbage: shuffled, overlapping and random tables - only the bounds are asked for (the sanitizer and the guard bands)
    for (int trial = 0; trial < 8; ++trial) {
        const int nr = (int)good.size();
        Banded<r3d_window_run_desc> tab((size_t)nr, good[0]);
        for (int i = 0; i < nr; ++i) tab[(size_t)i] = good[(size_t)((i * 7 + trial) % nr)];
        if (trial == 1)
            for (int i = 0; i < nr; ++i) tab[(size_t)i].win_first = 0;
        if (trial >= 2)
            for (int i = 0; i < nr; ++i) {
                uint32_t w[12];
                for (uint32_t &v : w) v = next(seed) >> (trial * 3);
                std::memcpy(&tab[(size_t)i], w, sizeof(w));
                if (trial & 1) {
                    tab[(size_t)i].first_frame = (int64_t)(next(seed) % (uint32_t)total);
                    tab[(size_t)i].n_frames = (int64_t)(next(seed) % 50u);
                    tab[(size_t)i].win_first = (int64_t)(next(seed) % 300u);
                    tab[(size_t)i].flip = (int32_t)(next(seed) % 3u);
                }
            }
        Banded<float> rp((size_t)nr * E, FILL), x((size_t)64 * RF * J * F, FILL), param((size_t)64 * E, FILL);
        Banded<int32_t> status((size_t)nr, -1);
        for (int64_t w0 : {(int64_t)0, (int64_t)100, (int64_t)1 << 40, (int64_t)1 << 62})
            EXPECT(r3d_debug_clips_windows_host(src.data(), total, J, F, RF, tab.data(), nr, rp.data(), E, w0, 64, x.data(), param.data(), perm, status.data()) == 0);
        EXPECT(src.guards_clean() && rp.guards_clean() && x.guards_clean() && param.guards_clean() && status.guards_clean() && tab.guards_clean());
    }
    // the argument rules: nothing may be written
    Banded<r3d_window_run_desc> tab(good.size(), good[0]);
    for (size_t i = 0; i < good.size(); ++i) tab[i] = good[i];
    const int nr = (int)good.size();
    Banded<float> rp((size_t)nr * E, FILL), x((size_t)8 * RF * J * F, FILL), param((size_t)8 * E, FILL);
    Banded<int32_t> status((size_t)nr, -1);
    int32_t twice[17];
    for (int j = 0; j < J; ++j) twice[j] = 0;
    const r3d_window_run_desc *t = tab.data();
#define CALL(S, TOT, JJ, FF, RR, TAB, NR, RP, EE, W0, B, X, P, PERM, ST) \
    EXPECT(r3d_debug_clips_windows_host(S, TOT, JJ, FF, RR, TAB, NR, RP, EE, W0, B, X, P, PERM, ST) == R3D_ERR_ARG)
    CALL(nullptr, total, J, F, RF, t, nr, rp.data(), E, 0, 8, x.data(), param.data(), perm, status.data());
    CALL(src.data(), total, J, F, RF, nullptr, nr, rp.data(), E, 0, 8, x.data(), param.data(), perm, status.data());
    CALL(src.data(), total, J, F, RF, t, nr, rp.data(), E, 0, 8, nullptr, param.data(), perm, status.data());
    CALL(src.data(), total, J, F, RF, t, nr, rp.data(), E, 0, 8, x.data(), param.data(), perm, nullptr);
    CALL(src.data(), total, J, F, RF, t, 0, rp.data(), E, 0, 8, x.data(), param.data(), perm, status.data());
    CALL(src.data(), total, J, F, RF, t, R3D_CLIPS_MAX + 1, rp.data(), E, 0, 8, x.data(), param.data(), perm, status.data());
    CALL(src.data(), total, 0, F, RF, t, nr, rp.data(), E, 0, 8, x.data(), param.data(), nullptr, status.data());
    CALL(src.data(), total, 18, F, RF, t, nr, rp.data(), E, 0, 8, x.data(), param.data(), nullptr, status.data());
    CALL(src.data(), total, J, 1, RF, t, nr, rp.data(), E, 0, 8, x.data(), param.data(), perm, status.data());
    CALL(src.data(), total, J, 4, RF, t, nr, rp.data(), E, 0, 8, x.data(), param.data(), perm, status.data());
    CALL(src.data(), total, J, F, 0, t, nr, rp.data(), E, 0, 8, x.data(), param.data(), perm, status.data());
    CALL(src.data(), 0, J, F, RF, t, nr, rp.data(), E, 0, 8, x.data(), param.data(), perm, status.data());
    CALL(src.data(), total, J, F, RF, t, nr, rp.data(), E, 0, 0, x.data(), param.data(), perm, status.data());
    CALL(src.data(), total, J, F, RF, t, nr, rp.data(), E, 0, 65536, x.data(), param.data(), perm, status.data());
    CALL(src.data(), total, J, F, RF, t, nr, rp.data(), E, -1, 8, x.data(), param.data(), perm, status.data());
    CALL(src.data(), total, J, F, RF, t, nr, rp.data(), E, ((int64_t)1 << 62) + 1, 8, x.data(), param.data(), perm, status.data());
    CALL(src.data(), total, J, F, R3D_ENCODE_MAX_POINTS / J + 1, t, nr, rp.data(), E, 0, 8, x.data(), param.data(), perm, status.data());
    CALL(src.data(), (int64_t)R3D_ENCODE_MAX_POINTS + 1, J, F, RF, t, nr, rp.data(), E, 0, 8, x.data(), param.data(), perm, status.data());
    CALL(src.data(), total, J, F, R3D_ENCODE_MAX_POINTS / J / 4, t, nr, rp.data(), E, 0, 8, x.data(), param.data(), perm, status.data());
    CALL(src.data(), total, J, F, RF, t, nr, nullptr, E, 0, 8, x.data(), param.data(), perm, status.data());
    CALL(src.data(), total, J, F, RF, t, nr, rp.data(), E, 0, 8, x.data(), nullptr, perm, status.data());
    CALL(src.data(), total, J, F, RF, t, nr, rp.data(), 0, 0, 8, x.data(), param.data(), perm, status.data());
    if (J > 1) CALL(src.data(), total, J, F, RF, t, nr, rp.data(), E, 0, 8, x.data(), param.data(), twice, status.data());
    CALL(src.data(), total, J, F, RF, reinterpret_cast<const r3d_window_run_desc *>(reinterpret_cast<const char *>(t) + 4), nr, rp.data(), E, 0, 8, x.data(),
         param.data(), perm, status.data());
#undef CALL
    for (size_t i = 0; i < x.n; ++i) EXPECT(x[i] == FILL);
    for (size_t i = 0; i < param.n; ++i) EXPECT(param[i] == FILL);
    for (size_t i = 0; i < status.n; ++i) EXPECT(status[i] == -1);
}

}  // namespace

int main() {
    for (int J : {1, 14, 17})
        for (int F : {2, 3})
            for (int m = 0; m < 8; ++m) run(J, F, m & 4 ? 27 : 9, m & 1, m & 2, (m >> 1 ^ m) & 1);
    if (failures) {
        std::fprintf(stderr, "%d expectation(s) failed\n", failures);
        return 1;
    }
    std::printf("san_clips_windows: ok\n");
    return 0;
}
