// Stand-alone driver of r3d_debug_pack_replay_host for `make san_pack_replay` (ray3d_amd/csrc/Makefile): linked against
// libray3d_hip_san.so - the host objects built -fsanitize=address,undefined - and built with the same flags itself, it runs the
// descriptor, inverse and segment tables of r3d_finalize_dev and the per-element routines of r3d_pack.hpp on HOST memory only (no
// device call, no GPU needed): index arithmetic over every element of a packed image, against exact-size heap blocks (the source
// tensors the library copies at r3d_set_weight, the two images) with the sanitizer's red zones around them.  Three configurations:
// FuseBlocks' four folded ranges with per-frame [E | V] layers and the bf16-operand-order copies; the dense ablation with two
// input features, no embedding and no shrink fold; a trajectory network.  The weights carry negated and zero gammas and
// variances far below the BatchNorm eps.  Also the argument rules of r3d_finalize_dev, which end before any device call.
// Exit status 0: every image bit for bit and no sanitizer report.
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
        std::fprintf(stderr, "san_pack_replay.cpp:%d: %s (%s)\n", line, what, r3d_last_error());
        ++failures;
    }
}
#define EXPECT(c) expect((c), #c, __LINE__)

float rnd(uint32_t &s) {
    s = s * 1664525u + 1013904223u;
    return (float)((s >> 8) & 0xffff) / 65536.0f - 0.5f;
}

bool ends_with(const char *s, const char *tail) {
    const size_t n = std::strlen(s), t = std::strlen(tail);
    return n >= t && std::strcmp(s + n - t, tail) == 0;
}

void run(const char *name, r3d_config cfg, uint32_t seed) {
    cfg.struct_size = (int32_t)sizeof(r3d_config);
    r3d_model *m = nullptr;
    EXPECT(r3d_create(&cfg, &m) == R3D_OK);
    if (!m) return;
    const int n = r3d_num_weights(m);
    EXPECT(n > 0);
    int64_t mism = -2, first = -2;
    EXPECT(r3d_debug_pack_replay_host(m, &mism, &first) == R3D_ERR_KEY);          // nothing set yet
    std::vector<int64_t> numel(n);
    for (int i = 0; i < n; ++i) {
        int64_t shape[4];
        int rank = 0;
        EXPECT(r3d_weight_shape(m, i, shape, &rank) == R3D_OK);
        int64_t count = 1;
        for (int d = 0; d < rank; ++d) count *= shape[d];
        numel[i] = count;
        const char *key = r3d_weight_key(m, i);
        std::vector<float> v((size_t)count);                                          // exact size: a read past it is a report
        const bool var = ends_with(key, ".running_var"), gamma = !var && std::strstr(key, "bn") && ends_with(key, ".weight");
        for (int64_t e = 0; e < count; ++e) {
            const float r = rnd(seed);
            if (var) v[e] = e % 7 == 0 ? 1e-9f : 1.0f + r;                             // some far below eps
            else if (gamma) v[e] = e % 11 == 0 ? 0.0f : e % 4 == 0 ? -(1.0f + 0.4f * r) : 1.0f + 0.4f * r;
            else v[e] = 0.2f * r;
        }
        EXPECT(r3d_set_weight(m, key, v.data(), shape, rank) == R3D_OK);
    }
    EXPECT(r3d_debug_pack_replay_host(m, &mism, &first) == R3D_OK);
    EXPECT(mism == 0 && first == -1);
    EXPECT(r3d_debug_pack_replay_host(m, nullptr, &first) == R3D_ERR_ARG);
    // r3d_finalize_dev's argument rules: answered before any device call (there is no device here)
    std::vector<const float *> ptrs(n, reinterpret_cast<const float *>(uintptr_t(0x1000)));
    EXPECT(r3d_finalize_dev(m, ptrs.data(), numel.data(), n - 1, nullptr) == R3D_ERR_ARG);
    EXPECT(r3d_finalize_dev(m, nullptr, numel.data(), n, nullptr) == R3D_ERR_ARG);
    EXPECT(r3d_finalize_dev(m, ptrs.data(), nullptr, n, nullptr) == R3D_ERR_ARG);
    ptrs[n / 2] = nullptr;
    EXPECT(r3d_finalize_dev(m, ptrs.data(), numel.data(), n, nullptr) == R3D_ERR_ARG && std::strstr(r3d_last_error(), r3d_weight_key(m, n / 2)));
    ptrs[n / 2] = ptrs[0];
    numel[n - 1] += 1;
    EXPECT(r3d_finalize_dev(m, ptrs.data(), numel.data(), n, nullptr) == R3D_ERR_SHAPE && std::strstr(r3d_last_error(), r3d_weight_key(m, n - 1)));
    std::printf("%-28s %4d tensors: %lld mismatches\n", name, n, (long long)mism);
    EXPECT(r3d_destroy(m) == R3D_OK);
}

}  // namespace

int main() {
    //                         kind           J   F  levels  C   latent stage E  D  causal dense b3
    run("j14-rf9-s3-bf16x3", {0, R3D_KIND_POS, 14, 3, 2, 64, 128, 3, 2, 64, 0, 0, 1}, 1u);
    run("j17-f2-rf27-dense-nofold", {0, R3D_KIND_POS, 17, 2, 3, 96, 64, 2, 0, 0, 0, 1, 0}, 2u);
    run("j15-rf27-trj", {0, R3D_KIND_TRJ, 15, 3, 3, 128, 128, 1, 2, 32, 1, 0, 0}, 3u);
    if (failures) {
        std::fprintf(stderr, "san_pack_replay: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("san_pack_replay: ok\n");
    return 0;
}
