// r3d_finalize_dev: the BatchNorm-folding repack of model_finalize (r3d_model.cpp) per destination element, __host__ __device__ so
// that the kernel (r3d_k_pack, r3d_k_elementwise.hip) and the hooks build's host replay
// (r3d_debug_pack_replay_host) run the very same routines.  The promise of include/ray3d_hip.h is an image that is bit for bit what
// r3d_finalize uploads, so every routine replays model_finalize's float64 arithmetic in its order:
//   * each host accumulator (rowacc[k], extra) is a chain of its own - one work item replays one chain, serially;
//   * floating-point contraction is OFF in every routine: the host objects are built for baseline x86-64 (no FMA), and a fused
//     multiply-add would round a product and a sum together;
//   * float64 sqrt and / are the IEEE correctly rounded operations on both sides.
// A work item is a QUAD: four consecutive GEMM columns k0 .. k0 + 3 of one output channel, which are 16 consecutive bytes in every
// layout of the arena (fragment order, row-major, bf16-operand order) - one 16-byte store per item, consecutive items at consecutive
// addresses.  The source reads are strided (a row of a torch tensor per output channel) and go through the caches.
//
// What drives it is a per-layer descriptor table (PackLayer, built once per handle from Model::layers by model_pack_tables), the
// inverse column table of the first layers and a segment list that cuts a flat grid into runs of workgroups per (layer, kind).
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace r3d {

constexpr int PACK_MAX_PRE = 4;        // folded input ranges of one layer (FuseBlocks' fc_1: the other four branches)
constexpr int PACK_THREADS = 256;      // work items per workgroup; every segment is a whole number of workgroups

// one shrink-folded input range (Layer::Pre): reference columns [ref_col0, ref_col0 + ref_width) of the layer's weight are the
// operand columns [k0, k0 + new_width): W[:, range] . S with S = tensor `sw` (ref_width, new_width), bias tensor `sb` (or -1)
struct PackPre { int ref_col0, ref_width, new_width, k0, sw, sb; };

struct PackLayer {
    // source tensors (indices into the caller's pointer table = r3d_weight_key order); -1: the layer has none
    int w, bias, g, beta, mu, var;      // weight, bias, BatchNorm weight / bias / running_mean / running_var   (cases 1-4)
    int N, Npad, Kpad;                  // output channels, padded rows and columns of the image                  (all cases)
    int taps, cin, cin_ref;             // torch layout (N, cin, taps); cin_ref: the reference width of a `pre` layer (cases 2-4)
    int frag;                           // 1: MFMA fragment order, 0: row-major [N][Kpad] (the decoder tails)    (cases 2, 3)
    int npre;                           // shrink-folded ranges                                                   (cases 1, 3)
    PackPre pre[PACK_MAX_PRE];
    int inv0;                           // first layers: where this layer's Kpad + 1 list starts begin in the inverse table; -1 (case 4)
    int shared_of, shared_split, src_N; // [E | V] per-frame layer: source layer (or -1), first current-frame column, its N (case 5)
    long long w_off, b_off, wb3_off;    // floats into the arena; wb3_off -1: no bf16-operand-order copy                (all / case 5)
    long long src_w_off, src_b_off;     // the source layer's image and bias (shared_of >= 0)                            (case 5)
};

// a run of workgroups: [blk0, blk0 + nblk) of the launch work on `kind` of layer `layer`
enum { PACK_BIAS = 0, PACK_WEIGHT = 1, PACK_SHARED_W = 2, PACK_SHARED_B = 3, PACK_BF3 = 4 };
struct PackSeg { int layer, kind, blk0, nblk; };

// the arguments of one launch of r3d_k_pack
struct PackArgs {
    const PackSeg *segs;
    int nseg;
    const PackLayer *layers;
    const int *inv;                     // first layers: per layer Kpad + 1 starts (absolute indices into inv), then the entries
                                        // (source index c * taps + tap) << 1 | subtract, in the host's visiting order
    const float *const *T;              // the caller's tensors, r3d_weight_key order
    float *arena;
};

__host__ __device__ inline size_t pack_frag_index(int o, int k, int nk) {      // frag_index of r3d_internal.hpp
    const int nb = o >> 5, li = o & 31, kt = k >> 5, kin = k & 31, lh = kin >> 4, q = (kin & 15) >> 2, e = kin & 3;
    return ((((size_t)nb * nk + kt) * 4 + q) * 64 + (lh * 32 + li)) * 4 + e;
}

// case 1: scale of output channel o (Folder::scale_shift)
__host__ __device__ inline double pack_scale(const PackLayer &L, const float *const *T, int o) {
#pragma clang fp contract(off)
    if (L.g < 0) return 1.0;
    return (double)T[L.g][o] / sqrt((double)T[L.var][o] + 1e-5);
}

// case 1: shift of output channel o, the `pre` layers' extra term included, cast as the bias is stored
__host__ __device__ inline float pack_shift(const PackLayer &L, const float *const *T, int o, double s) {
#pragma clang fp contract(off)
    const float *bias = L.bias >= 0 ? T[L.bias] : nullptr;
    double t;
    if (L.g < 0)
        t = bias ? (double)bias[o] : 0.0;
    else
        t = (double)T[L.beta][o] - (double)T[L.mu][o] * s + (bias ? (double)bias[o] * s : 0.0);
    if (L.npre > 0) {
        const float *w = T[L.w] + (size_t)o * L.cin_ref;
        double extra = 0.0;
        for (int r = 0; r < L.npre; ++r) {
            const PackPre &p = L.pre[r];
            if (p.sb < 0) continue;
            const float *sb = T[p.sb];
            for (int q = 0; q < p.ref_width; ++q) extra += (double)w[p.ref_col0 + q] * (double)sb[q];
        }
        t += extra * s;
    }
    return (float)t;
}

// case 3: one column of a `pre` layer: inside folded range r the q-ordered sum, outside it the reference column that lands there
__host__ __device__ inline float pack_pre_column(const PackLayer &L, const float *const *T, int o, int k, double s) {
#pragma clang fp contract(off)
    const float *w = T[L.w] + (size_t)o * L.cin_ref;
    int c = 0, kk = 0;                  // reference column / operand column where the identity run in front of range r starts
    for (int r = 0; r <= L.npre; ++r) {
        const int run = (r < L.npre ? L.pre[r].ref_col0 : L.cin_ref) - c;
        if (k < kk + run) return (float)((double)w[c + (k - kk)] * s);
        if (r == L.npre) break;
        const PackPre &p = L.pre[r];
        c += run;
        kk += run;
        if (k < kk + p.new_width) {
            const float *sw = T[p.sw] + (k - kk);
            double acc = 0.0;
            for (int q = 0; q < p.ref_width; ++q) acc += (double)w[c + q] * (double)sw[(size_t)q * p.new_width];
            return (float)(acc * s);
        }
        c += p.ref_width;
        kk += p.new_width;
    }
    return (float)(0.0 * s);            // a padding column: the host casts its untouched accumulator times s
}

// cases 2-4: the quad (o, k0 .. k0 + 3) of a layer with tensors of its own
__host__ __device__ inline void pack_quad(const PackLayer &L, const float *const *T, const int *inv, int o, int k0, float out[4]) {
#pragma clang fp contract(off)
    out[0] = out[1] = out[2] = out[3] = 0.0f;
    if (o >= L.N) return;               // padding rows stay zero
    const double s = pack_scale(L, T, o);
    if (L.npre > 0) {
        // the four columns of a quad inside one folded range share the walk over q (four chains side by side)
        for (int r = 0; r < L.npre; ++r) {
            const PackPre &p = L.pre[r];
            if (k0 >= p.k0 && k0 + 3 < p.k0 + p.new_width) {
                const float *w = T[L.w] + (size_t)o * L.cin_ref + p.ref_col0;
                const float *sw = T[p.sw] + (k0 - p.k0);
                double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
                for (int q = 0; q < p.ref_width; ++q) {
                    const double wq = (double)w[q];
                    const float *srow = sw + (size_t)q * p.new_width;
                    a0 += wq * (double)srow[0];
                    a1 += wq * (double)srow[1];
                    a2 += wq * (double)srow[2];
                    a3 += wq * (double)srow[3];
                }
                out[0] = (float)(a0 * s);
                out[1] = (float)(a1 * s);
                out[2] = (float)(a2 * s);
                out[3] = (float)(a3 * s);
                return;
            }
        }
        for (int e = 0; e < 4; ++e) out[e] = pack_pre_column(L, T, o, k0 + e, s);
        return;
    }
    if (L.inv0 < 0) {                   // case 2: GEMM column k = tap * cin + c of torch element (o, c, tap)
        const float *w = T[L.w] + (size_t)o * L.cin * L.taps;
        for (int e = 0; e < 4; ++e) {
            const int k = k0 + e;
            if (k >= L.taps * L.cin) break;
            const int j = k / L.cin, c = k - j * L.cin;
            out[e] = (float)((double)w[(size_t)c * L.taps + j] * s);
        }
        return;
    }
    // case 4: the operand column's sources, added and subtracted in the host's visiting order
    const float *w = T[L.w] + (size_t)o * L.cin * L.taps;
    const int *start = inv + L.inv0;
    for (int e = 0; e < 4; ++e) {
        double acc = 0.0;
        for (int i = start[k0 + e]; i < start[k0 + e + 1]; ++i) {
            const double v = (double)w[inv[i] >> 1] * s;
            if (inv[i] & 1) acc -= v;
            else acc += v;
        }
        out[e] = (float)acc;
    }
}

// where quad `qi` of a fragment-ordered or row-major image of Kpad columns lies: its output channel and first column
__host__ __device__ inline void pack_quad_place(int frag, int Kpad, int qi, int &o, int &k0) {
    if (!frag) {
        o = qi / (Kpad / 4);
        k0 = (qi - o * (Kpad / 4)) * 4;
        return;
    }
    const int nk = Kpad / 32, lane = qi & 63, q = (qi >> 6) & 3, rest = qi >> 8, kt = rest % nk, nb = rest / nk;
    o = nb * 32 + (lane & 31);
    k0 = kt * 32 + (lane >> 5) * 16 + q * 4;
}

__host__ __device__ inline void pack_store4(float *dst, const float v[4]) {
    *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
}

// One work item of segment `sg`: item < nblk * PACK_THREADS.  Every store lies inside the layer's own image: a weight / copy
// segment has Npad * Kpad / 4 items of 4 floats, a bias segment Npad items of one.
__host__ __device__ inline void pack_item(const PackArgs &a, const PackSeg &sg, int item) {
    const PackLayer &L = a.layers[sg.layer];
    float v[4];
    switch (sg.kind) {
        case PACK_BIAS:
            a.arena[L.b_off + item] = item < L.N ? pack_shift(L, a.T, item, pack_scale(L, a.T, item)) : 0.0f;
            return;
        case PACK_WEIGHT: {
            int o, k0;
            pack_quad_place(L.frag, L.Kpad, item, o, k0);
            pack_quad(L, a.T, a.inv, o, k0, v);
            pack_store4(a.arena + L.w_off + 4 * (size_t)item, v);
            return;
        }
        case PACK_SHARED_W: {           // case 5: [E | V] from the source layer's fragment-ordered image
            int o, k0;
            pack_quad_place(1, L.Kpad, item, o, k0);
            const int C = L.src_N, half = o >= C, so = half ? o - C : o;
            for (int e = 0; e < 4; ++e) {
                const bool keep = o < 2 * C && ((k0 + e < L.shared_split) != (half != 0));
                v[e] = keep ? a.arena[L.src_w_off + pack_frag_index(so, k0 + e, L.Kpad / 32)] : 0.0f;
            }
            pack_store4(a.arena + L.w_off + 4 * (size_t)item, v);
            return;
        }
        case PACK_SHARED_B:
            a.arena[L.b_off + item] = item < L.src_N ? a.arena[L.src_b_off + item] : 0.0f;
            return;
        case PACK_BF3: {                // case 5: the layer's own image in v_mfma_f32_32x32x16_bf16 operand order
            const int nk = L.Kpad / 32, lane = item & 63, j = (item >> 6) & 1, h = (item >> 7) & 1, rest = item >> 8;
            const int kt = rest % nk, nb = rest / nk, o = nb * 32 + (lane & 31), k0 = kt * 32 + h * 16 + (lane >> 5) * 8 + j * 4;
            for (int e = 0; e < 4; ++e) v[e] = o < L.N ? a.arena[L.w_off + pack_frag_index(o, k0 + e, nk)] : 0.0f;
            pack_store4(a.arena + L.wb3_off + 4 * (size_t)item, v);
            return;
        }
        default: return;
    }
}

}  // namespace r3d
