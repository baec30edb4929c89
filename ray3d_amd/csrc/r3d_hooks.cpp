// The r3d_debug_* exports of libray3d_hip_hooks.so: checkers that run on the host and never touch a device (one exception, at the
// end: r3d_debug_weights_image copies the packed image back).
#ifdef R3D_TEST_HOOKS      // (libray3d_hip_hooks.so only: the product library gets an empty translation unit)
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <set>
#include <utility>

#include "r3d_internal.hpp"
#include "r3d_clips_repair.hpp"
#include "r3d_poses.hpp"
#include "r3d_project.hpp"
#include "r3d_streams.hpp"
#include "r3d_streams_assign.hpp"
#include "r3d_streams_fuse.hpp"
#include "r3d_streams_link.hpp"
#include "r3d_streams_peek.hpp"
#include "r3d_streams_poses.hpp"
#include "r3d_streams_repair.hpp"
#include "r3d_undistort.hpp"
#include "r3d_valid.hpp"
#include "r3d_windows.hpp"

using namespace r3d;

namespace {

// ---- r3d_debug_forward_census: the one restatement of device code in this file.
// What the persistent loop's dispatch reads of a tile: its problem's operand pointers (set or not) and K, the tile's
// units (mi) and code (ks); and of its kernel: the template arguments of gemm_persistent (r3d_k_*.hip).
struct CensusProb { bool w3, lut, wb3, w2; int K; };
struct CensusKernel { const char *name; bool enc, uv, dep, b3, narrow, clip; };

std::vector<CensusKernel> census_kernels() {
    std::vector<CensusKernel> v;
    for (int uv = 0; uv < 2; ++uv) {
        const bool u = uv != 0;
        // r3d_k_gemm.hip, r3d_k_gemm_enc.hip, r3d_k_gemm_b3.hip: gemm_persistent<ENC, UV, DEP = false, B3[, NARROW]>, CLIP = !DEP
        v.push_back({stage_kernel_name(STAGE_BIG, u, false), false, u, false, false, true, true});
        v.push_back({stage_kernel_name(STAGE_ENC, u, false), true, u, false, false, false, true});
        v.push_back({stage_kernel_name(STAGE_BIG, u, true), false, u, false, true, true, true});
        // r3d_k_fwd_*.hip: R3D_FORWARD_KERNEL(name, UV, B3, NARROW, CLIP) = gemm_persistent<false, UV, true, B3, NARROW, CLIP>
        v.push_back({forward_kernel_name(FWD_KERNEL_F32, u), false, u, true, false, false, false});
        v.push_back({forward_kernel_name(FWD_KERNEL_B3, u), false, u, true, true, false, false});
        v.push_back({forward_kernel_name(FWD_KERNEL_LAT, u), false, u, true, false, true, false});
        v.push_back({forward_kernel_name(FWD_KERNEL_CLIP, u), false, u, true, false, false, true});
    }
    return v;
}

// The tile function and template arguments gemm_persistent's dispatch (r3d_tiles.hpp, the do { } while (false) block of the
// persistent loop) selects for one tile, as the switches clamp them.  Keep the two in step: a tile kind added there is
// added here, and tests/test_specialisations_host.py then asks for a case that reaches it.
std::string census_tile_kind(const CensusKernel &k, const CensusProb &P, int mi, int ks) {
    char b[48];
    const char *in = k.uv ? "UV" : "rays";
    auto enc = [&] { snprintf(b, sizeof b, "enc_tile<%d,%s>", mi == 1 ? 1 : mi == 2 ? 2 : 3, in); return std::string(b); };
    if (k.enc) return enc();
    if (P.w3) {                                  // the fused first level
        const int m = mi >= 2 ? 2 : 1;
        if (k.clip && !P.lut) snprintf(b, sizeof b, "first_level_shared<%d>", m);
        else snprintf(b, sizeof b, "first_level_taps%s<%d,%s,%s>", k.b3 && P.wb3 ? "_b3" : "", m, P.K <= 64 ? "K<=64" : "K>64", in);
        return b;
    }
    if (P.lut) return enc();
    if (k.b3 && P.wb3 && P.w2) { snprintf(b, sizeof b, "gemm_tile_b3t<%d>", mi >= 3 ? 3 : mi == 2 ? 2 : 1); return b; }
    if (k.b3 && P.wb3) {
        if (mi == 1) return "gemm_tile_b3p<1>";
        snprintf(b, sizeof b, "gemm_tile_b3<%d>", mi == 2 ? 2 : mi == 3 ? 3 : 4);
        return b;
    }
    if (k.narrow && ks == 8) return k.dep ? "gemv_run" : "gemv_tile";
    if (k.narrow && ks == 16) return "lat_tile";
    if (ks > NB_CODE) { snprintf(b, sizeof b, "gemm_tile_nb<%d>", ks == NB_CODE + 4 ? 4 : ks == NB_CODE + 5 ? 5 : ks == NB_CODE + 6 ? 6 : 7); return b; }
    if (ks > 1) return ks == 4 ? "gemm_tile<1,4>" : mi == 1 ? "gemm_tile<1,2>" : "gemm_tile<2,2>";
    if (P.w2) { snprintf(b, sizeof b, "gemm_tile<%d,1,pair>", mi >= 1 && mi <= 3 ? mi : 4); return b; }
    snprintf(b, sizeof b, "gemm_tile<%d,1>", mi >= 1 && mi <= 5 ? mi : 6);
    return b;
}

const CensusKernel *census_find(const std::vector<CensusKernel> &ks, const char *name) {
    for (const CensusKernel &k : ks)
        if (!strcmp(k.name, name)) return &k;
    return nullptr;
}

CensusProb census_prob(const unsigned char *tg, int K) {       // (fill_prob's base tags: which pointer fields are set)
    return {tg[13] != BIND_NULL, tg[15] != BIND_NULL, tg[10] != BIND_NULL, tg[8] != BIND_NULL, K};
}

struct CensusOut {
    r3d_census_row *rows;
    int cap, n = 0, launch = 0;
    void row(const char *kernel, int blocks, const char *kind, int tiles) {
        if (n < cap) {
            r3d_census_row &r = rows[n];
            memset(&r, 0, sizeof r);
            r.launch = launch;
            r.blocks = blocks;
            r.tiles = tiles;
            strncpy(r.kernel, kernel, sizeof r.kernel - 1);
            strncpy(r.tile_kind, kind, sizeof r.tile_kind - 1);
        }
        ++n;
    }
    void launch_of(const char *kernel, int blocks, const std::map<std::string, int> &hist) {
        if (hist.empty()) row(kernel, blocks, "", 0);
        for (const auto &kv : hist) row(kernel, blocks, kv.first.c_str(), kv.second);
        ++launch;
    }
};

// the host part of a schedule (what schedule_get builds before it touches the device), kept for the last (pair, plan, B, nwg)
// asked: a sweep asks every call shape of a size in a row.  (Handles are keyed by their never-reused ids; a development switch
// that changes the tile lists - R3D_NO_GEMV, R3D_NO_NB, ... - is set before a pair's first census, like before its first forward.)
struct CensusSched {
    uint64_t ida = 0, idb = 0;
    const Plan *pl = nullptr;
    int64_t B = -1;
    int nwg = 0;
    int spill_row0 = -1;
    std::vector<int4> tiles;
    std::vector<int> wgoff;
    std::vector<StageSchedule> stages;
    const std::vector<std::vector<int>> *levels = nullptr;
    Schedule::Fwd fw;
    std::vector<int> ft, fo;
};
thread_local CensusSched g_census;

}  // namespace

extern "C" {

// Test hook: build the static schedule of one launch on the host and verify
// that its tiles cover every (32-row unit, 32-column granule) of every problem exactly once within the
// kernel's tile-shape limits.  Returns 0 or a negative code naming the first violated rule.
int r3d_debug_schedule_check(int nprob, const int *M, const int *N, const int *nk, const int *max_ks, const int *max_units,
                             int nwg, int enc, int *out_grid, int *out_tiles, double *out_imbalance) {
    std::vector<SchedProb> probs;
    for (int i = 0; i < nprob; ++i) {
        probs.push_back({M[i], N[i], nk[i], max_ks[i], max_units[i]});
        // (as sched_prob_of marks the plan's wide plain layers: their single-unit tiles may be 4 .. 7 column blocks wide)
        probs.back().nb_ok = !enc && N[i] % 32 == 0 && N[i] >= 512 && nk[i] >= 8 && max_units[i] == 0 && !hook_on("R3D_NO_NB");
        probs.back().run_ok = probs.back().nb_ok;
    }
    std::vector<int4> tiles;
    std::vector<int> wgoff;
    StageSchedule ss{};
    schedule_stage(probs, nwg, GEMM_SCHED_MAX_UNITS, tiles, wgoff, ss, enc != 0);
    if (out_grid) *out_grid = ss.nwg;
    if (out_tiles) *out_tiles = ss.ntiles;
    if (out_imbalance) *out_imbalance = ss.imbalance;
    if (ss.nwg < 1 || ss.nwg > nwg) return -1;
    if ((int)wgoff.size() != ss.nwg + 1 || wgoff.front() != 0 || wgoff.back() != ss.ntiles || (int)tiles.size() != ss.ntiles) return -2;
    for (size_t i = 1; i < wgoff.size(); ++i)
        if (wgoff[i] <= wgoff[i - 1] && ss.ntiles > 0) return -3;          // empty or unordered chunk
    std::vector<std::vector<int>> cover(nprob);
    for (int i = 0; i < nprob; ++i) cover[i].assign((size_t)((M[i] + 31) / 32) * ((N[i] + COL_GRANULE - 1) / COL_GRANULE), 0);
    for (const int4 &t : tiles) {
        const int pi = t.x & 0xff, mi = tile_units(t.x), ks = t.w;
        if (tile_src2(t.x) >= 0) {                 // a two-source tile: one unit, the rest of its row and the start of the next source's
            const int p2 = tile_src2(t.x);
            if (!tile_is_nb(ks) || mi != 1 || pi >= nprob || p2 >= nprob || t.z < 0 || t.z % 32 || t.z >= N[pi] || t.z + tile_width(ks) <= N[pi]) return -7;
            if (t.y % 32 || t.y < 0 || t.y >= M[pi] || nk[p2] != nk[pi]) return -7;
            TileSrc src[2];
            tile_sources(t.x, t.y, t.z, ks, N[pi], src);
            if (src[1].row0 >= M[p2] || src[1].cols > N[p2] || (p2 == pi ? false : t.y + 32 < M[pi])) return -7;
            for (const TileSrc &sc : src) {
                const int gc = (N[sc.prob] + COL_GRANULE - 1) / COL_GRANULE;
                for (int g = sc.col0 / COL_GRANULE; g < (sc.col0 + sc.cols) / COL_GRANULE; ++g) ++cover[sc.prob][(size_t)(sc.row0 / 32) * gc + g];
            }
            continue;
        }
        if (pi >= nprob || mi < 1 || (ks != 1 && ks != 2 && ks != 4 && ks != 8 && ks != 16 && !(ks >= NB_CODE + 4 && ks <= NB_CODE + 7))) return -4;
        if (ks < 8 && ks > max_ks[pi]) return -5;
        if ((ks == 1 && mi > (max_units[pi] > 0 ? std::min(max_units[pi], GEMM_SCHED_MAX_UNITS) : GEMM_SCHED_MAX_UNITS)) || (ks == 2 && mi > 2) || (ks >= 4 && mi != 1)) return -6;
        if (t.y % 32 || t.y < 0 || t.y >= M[pi] || t.z % (tile_is_nb(ks) ? 32 : tile_width(ks)) || t.z < 0 || t.z >= N[pi]) return -7;
        if (tile_is_nb(ks) && t.z + tile_width(ks) > N[pi]) return -7;        // (narrow tiles cover whole blocks of existing columns)
        if (ks > 1 && ks < 8 && (nk[pi] + ks - 1) / ks < 2) return -8;
        const int gcols = (N[pi] + COL_GRANULE - 1) / COL_GRANULE;
        for (int u = t.y / 32; u < t.y / 32 + mi; ++u) {
            if (u * 32 >= M[pi]) return -9;
            for (int g = t.z / COL_GRANULE; g < (t.z + tile_width(ks)) / COL_GRANULE && g < gcols; ++g) ++cover[pi][(size_t)u * gcols + g];
        }
    }
    for (int i = 0; i < nprob; ++i)
        for (int c : cover[i])
            if (c != 1) return -10;
    return 0;
}

// Test hook: the whole forward's tile lists for `batch` windows on `nwg` CUs, built on the host (no device needed):
// every 32-row x 32-column cell of every problem must be computed exactly once over all launches, a problem's
// tiles must sit in launches that list it, and a consumer's launch must come after all of its producers' tiles.
// Returns 0, or a negative code; *spilled = rows of the first level that run one launch late.
int r3d_debug_plan_check(r3d_model *pos, r3d_model *trj, int64_t batch, int nwg, int *launches, int *spilled) {
    const ModelPair mp = model_pair(pos, trj);
    Model *a = mp.a, *b = mp.b;
    if (!a) return -1;
    Plan *pl = plan_get(a, b, plan_kind(batch));
    if (!pl) return -2;
    int spill_row0 = -1;
    std::vector<int4> tiles;
    std::vector<int> wgoff;
    std::vector<StageSchedule> stages;
    const std::vector<std::vector<int>> &levels = *schedule_build_host(pl, batch, nwg, spill_row0, tiles, wgoff, stages);
    if (launches) *launches = (int)stages.size();
    if (spilled) *spilled = 0;
    const int np = (int)pl->probs.size();
    std::vector<std::vector<int>> cover(np);
    std::vector<int> last_launch(np, -1), first_launch(np, 1 << 30);
    for (int i = 0; i < np; ++i) {
        const ProbSpec &q = pl->probs[i];
        const int M = (int)(batch * q.rows_per_window), N = pl->m[q.model]->layers[q.layer].N;
        cover[i].assign((size_t)((M + 31) / 32) * ((N + COL_GRANULE - 1) / COL_GRANULE), 0);
    }
    for (size_t si = 0; si < stages.size(); ++si) {
        const StageSchedule &ss = stages[si];
        const auto &st = levels[si];
        if (ss.nwg < 1 || ss.nwg > 2 * nwg) return -3;
        {   // a launch runs ONE kernel: its problems are all r3d_gemm_enc_f32's or none is
            int n_enc = 0;
            for (int e : st) n_enc += pl->probs[e & ~STAGE_SPILL_IN].enc_kernel ? 1 : 0;
            if (n_enc != 0 && n_enc != (int)st.size()) return -11;
            if ((n_enc != 0) != (ss.kind == STAGE_ENC)) return -12;
        }
        for (int t = 0; t < ss.ntiles; ++t) {
            const int4 &tl = tiles[ss.tiles_off + t];
            const int slot = tl.x & 0xff, mi = tile_units(tl.x), ks = tl.w;
            if (slot >= (int)st.size() || mi < 1 || tile_src2(tl.x) >= (int)st.size()) return -4;
            const int id = st[slot] & ~STAGE_SPILL_IN;
            const ProbSpec &q = pl->probs[id];
            const int M = (int)(batch * q.rows_per_window), N = pl->m[q.model]->layers[q.layer].N;
            if (tl.y % 32 || tl.y < 0 || tl.y >= M || tl.z < 0 || tl.z >= N) return -5;
            if (id == pl->spill_prob) {
                const bool late = (st[slot] & STAGE_SPILL_IN) != 0;
                if (spill_row0 < 0 ? late : (late != (tl.y >= spill_row0))) return -6;
                if (late && spilled) *spilled += std::min(mi * 32, M - tl.y);
            }
            const int gcols = (N + COL_GRANULE - 1) / COL_GRANULE;
            for (int u = tl.y / 32; u < tl.y / 32 + mi; ++u) {
                if (u * 32 >= M) return -7;
                for (int g = tl.z / COL_GRANULE; g < (tl.z + tile_width(ks)) / COL_GRANULE && g < gcols; ++g) ++cover[id][(size_t)u * gcols + g];
            }
            last_launch[id] = std::max(last_launch[id], (int)si);
            first_launch[id] = std::min(first_launch[id], (int)si);
            if (tile_src2(tl.x) >= 0) {            // the second source of a two-source tile: the first blocks of one more unit
                TileSrc src[2];
                tile_sources(tl.x, tl.y, tl.z, ks, N, src);
                const int id2 = st[src[1].prob] & ~STAGE_SPILL_IN;
                const ProbSpec &q2 = pl->probs[id2];
                const int M2 = (int)(batch * q2.rows_per_window), N2 = pl->m[q2.model]->layers[q2.layer].N;
                if (!tile_is_nb(ks) || mi != 1 || (st[src[1].prob] & STAGE_SPILL_IN) || src[1].row0 >= M2 || src[1].cols > N2 || src[1].cols <= 0) return -5;
                const int gc2 = (N2 + COL_GRANULE - 1) / COL_GRANULE;
                for (int g = 0; g < src[1].cols / COL_GRANULE; ++g) ++cover[id2][(size_t)(src[1].row0 / 32) * gc2 + g];
                last_launch[id2] = std::max(last_launch[id2], (int)si);
                first_launch[id2] = std::min(first_launch[id2], (int)si);
            }
        }
    }
    for (int i = 0; i < np; ++i) {
        for (int c : cover[i])
            if (c != 1) return -8;
        for (int d : pl->probs[i].deps)
            if (last_launch[d] >= first_launch[i]) return -9;
    }
    return 0;
}

// Test hook: the single-launch form of the forward for `batch` windows on `nwg` CUs, built and EXECUTED on the host as a
// dependency machine: a workgroup's next tile runs when the ready counters it waits for are full; every tile must get to
// run (no waiting cycle), every counter must end full, and - independently of the dependency ranges the scheduler wrote -
// at the moment a tile runs, every earlier problem that writes what the tile reads, or reads / writes what the tile
// writes (same buffer, overlapping columns), must be complete for the tile's windows.
// Returns 0 (or 1: this plan runs launch by launch, nothing to check), or a negative code.  For the plan of calls of a few
// windows also: every workspace element is written exactly once per call (what poll mode relies on).
int r3d_debug_forward_check(r3d_model *pos, r3d_model *trj, int64_t batch, int nwg, int *out_tiles, int *out_counters) {
    const ModelPair mp = model_pair(pos, trj);
    Model *a = mp.a, *b = mp.b;
    if (!a) return -1;
    Plan *pl = plan_get(a, b, plan_kind(batch));
    int spill_row0 = -1;
    std::vector<int4> tiles;
    std::vector<int> wgoff;
    std::vector<StageSchedule> stages;
    const std::vector<std::vector<int>> &levels = *schedule_build_host(pl, batch, nwg, spill_row0, tiles, wgoff, stages);
    Schedule::Fwd fw;
    std::vector<int> ft, fo;
    if (!schedule_build_fwd(pl, batch, nwg, levels, stages, tiles, wgoff, fw, ft, fo)) return 1;
    if (out_tiles) *out_tiles = fw.ntiles;
    if (out_counters) *out_counters = fw.ncnt;
    const int np = (int)pl->probs.size(), TI = FWD_TILE_INT4 * 4;
    std::vector<int> gcols(np);
    for (int i = 0; i < np; ++i) gcols[i] = (pl->m[pl->probs[i].model]->layers[pl->probs[i].layer].N + COL_GRANULE - 1) / COL_GRANULE;
    std::vector<unsigned> cnt(fw.ncnt, 0);
    // column range a problem reads / writes in a workspace buffer
    struct Acc { int buf, c0, c1; };
    auto reads = [&](const ProbSpec &q) {
        std::vector<Acc> v;
        for (int sgi = 0; sgi < q.nseg; ++sgi)
            if (pl->buffers[q.seg[sgi].buf].external == 0) v.push_back({q.seg[sgi].buf, q.seg[sgi].col, q.seg[sgi].col + q.seg[sgi].width});
        if (q.res_buf >= 0) v.push_back({q.res_buf, q.res_col, q.res_col + pl->m[q.model]->layers[q.layer2 >= 0 && q.layer3 < 0 ? q.layer2 : q.layer].N});
        return v;
    };
    auto writes = [&](const ProbSpec &q) {
        const int N = pl->m[q.model]->layers[q.layer3 >= 0 ? q.layer3 : q.layer2 >= 0 ? q.layer2 : q.layer].N;
        return Acc{q.c_buf, q.c_col, q.c_col + N};
    };
    auto overlap = [](const Acc &x, const Acc &y) { return x.buf == y.buf && x.c0 < y.c1 && y.c0 < x.c1; };
    auto complete = [&](int prob, int w0, int w1) {           // every unit of `prob` that holds rows of windows [w0, w1)
        const ProbSpec &q = pl->probs[prob];
        const int M = (int)(batch * q.rows_per_window);
        const int a0 = w0 * q.rows_per_window, a1 = std::min(w1 * q.rows_per_window, M);
        for (int u = a0 / 32; u < (a1 + 31) / 32; ++u)
            if (cnt[fw.cnt_base[prob] + u] != (unsigned)gcols[prob]) return false;
        return true;
    };
    if (pl->kind == PLAN_SMALL) {
        // Calls of a few windows may take data as its own ready flag (poll mode): no element of a workspace buffer may then
        // be written twice in a call (a stale value would pass for data), and everything a problem reads from the workspace
        // must be written by some problem (a sentinel nobody replaces would be waited for until the spins give up).
        for (int i = 0; i < np; ++i)
            for (int o = 0; o < i; ++o)
                if (overlap(writes(pl->probs[i]), writes(pl->probs[o]))) return -25;
        // (column-exact where reader and writer see the buffer with the same row geometry - the MLPs' concatenations; a
        // pyramid level reads three of its producer's rows as one, there only "somebody writes this buffer" is checked)
        for (int i = 0; i < np; ++i)
            for (const Acc &rd : reads(pl->probs[i])) {
                std::vector<char> covered(rd.c1 - rd.c0, 0);
                bool any = false, same_rows = true;
                for (int o = 0; o < np; ++o) {
                    const Acc w = writes(pl->probs[o]);
                    if (w.buf != rd.buf) continue;
                    any = true;
                    same_rows = same_rows && pl->probs[o].rows_per_window == pl->probs[i].rows_per_window;
                    for (int c = std::max(w.c0, rd.c0); c < std::min(w.c1, rd.c1); ++c) covered[c - rd.c0] = 1;
                }
                if (!any) return -26;
                if (same_rows)
                    for (char c : covered)
                        if (!c) return -26;
            }
    }
    std::vector<int> next(fw.grid);
    for (int w = 0; w < fw.grid; ++w) next[w] = fo[w];
    int done = 0;
    for (bool progress = true; progress;) {
        progress = false;
        for (int w = 0; w < fw.grid; ++w) {
            while (next[w] < fo[w + 1]) {
                const int *d = &ft[(size_t)next[w] * TI];
                bool ready = true;
                for (int k = 0; k < d[4] && ready; ++k) {
                    const int base = d[8 + 2 * k], n = d[9 + 2 * k] & 0xffff;
                    const unsigned need = (unsigned)d[9 + 2 * k] >> 16;
                    for (int u = 0; u < n && ready; ++u) ready = cnt[base + u] >= need;
                }
                if (!ready) break;
                const int mi = tile_units(d[0]);
                TileSrc src[2];           // (a two-source tile: both sources' hazards, both sources' counters)
                const int nsrc = tile_sources(d[0], d[1], d[2], d[3], pl->m[pl->probs[d[0] & 0xff].model]->layers[pl->probs[d[0] & 0xff].layer].N, src);
                for (int sc = 0; sc < nsrc; ++sc) {
                    const int id = src[sc].prob;
                    const ProbSpec &q = pl->probs[id];
                    const int M = (int)(batch * q.rows_per_window);
                    if (src[sc].row0 >= M) return -21;
                    const int r1 = std::min(src[sc].row0 + mi * 32, M);
                    const int w0 = src[sc].row0 / q.rows_per_window, w1 = (r1 - 1) / q.rows_per_window + 1;
                    const Acc wr = writes(q);
                    for (int o = 0; o < id; ++o) {                 // (problems are created in the reference's execution order)
                        const ProbSpec &oq = pl->probs[o];
                        bool hazard = false;
                        for (const Acc &rd : reads(q)) hazard = hazard || overlap(rd, writes(oq));        // read after write
                        for (const Acc &rd : reads(oq)) hazard = hazard || overlap(rd, wr);               // write after read
                        hazard = hazard || overlap(writes(oq), wr);                                      // write after write
                        if (hazard && !complete(o, w0, w1)) return -20;
                    }
                    const int c0 = sc == 0 ? d[5] : d[7] >> 8, add = sc == 0 ? d[6] : src[1].cols / COL_GRANULE;
                    if (nsrc == 2 && (mi != 1 || !tile_is_nb(d[3]) || src[sc].cols <= 0 || src[sc].cols % COL_GRANULE || (sc == 0 && d[6] != src[0].cols / COL_GRANULE))) return -21;
                    if (c0 != fw.cnt_base[id] + src[sc].row0 / 32 || c0 + mi > fw.ncnt) return -21;
                    for (int u = 0; u < mi; ++u) {
                        cnt[c0 + u] += (unsigned)add;
                        if (cnt[c0 + u] > (unsigned)gcols[id]) return -22;
                    }
                }
                ++next[w];
                ++done;
                progress = true;
            }
        }
    }
    if (done != fw.ntiles) return -23;                          // a waiting cycle
    for (int i = 0; i < np; ++i)
        for (int u = 0; u < (int)((batch * pl->probs[i].rows_per_window + 31) / 32); ++u)
            if (cnt[fw.cnt_base[i] + u] != (unsigned)gcols[i]) return -24;
    return 0;
}

// Test hook: census of kernel specialisations (include/ray3d_hip.h).  Plan, tile lists, kernel choice and call form are the
// driver's own code (plan_kind, schedule_build_host, schedule_build_fwd, forward_kernel_of_lists, forward_variant_table,
// call_shares_first_layers, call_is_single, fill_prob, the *_kernel_name functions); only census_tile_kind restates device code.
int r3d_debug_forward_census(r3d_model *pos, r3d_model *trj, int64_t batch, int nwg, int32_t uv, int64_t cam_stride, int64_t window_stride,
                             int32_t staged, int32_t captured, r3d_census_row *rows, int32_t cap) {
    const ModelPair mp = model_pair(pos, trj);
    Model *a = mp.a, *b = mp.b;
    if (!a || batch <= 0 || nwg <= 0 || window_stride <= 0 || (!rows && cap > 0)) return -1;
    if (b && !same_input_shape(a, b)) return -1;
    if (uv && a->cfg.in_features != 3) return -1;              // (check_call: R3D_INPUT_UV needs three input features)
    Plan *pl = plan_get(a, b, plan_kind(batch));
    if (!pl) return -2;
    CensusSched &cs = g_census;
    if (cs.ida != a->id || cs.idb != (b ? b->id : 0) || cs.pl != pl || cs.B != batch || cs.nwg != nwg) {
        cs = CensusSched();
        cs.ida = a->id;
        cs.idb = b ? b->id : 0;
        cs.pl = pl;
        cs.B = batch;
        cs.nwg = nwg;
        cs.levels = schedule_build_host(pl, batch, nwg, cs.spill_row0, cs.tiles, cs.wgoff, cs.stages);
        if (forward_single_launch() && schedule_build_fwd(pl, batch, nwg, *cs.levels, cs.stages, cs.tiles, cs.wgoff, cs.fw, cs.ft, cs.fo)) {
            bool narrow = false, b3_tiles = false;
            cs.fw.kernel = forward_kernel_of_lists(pl, batch, cs.ft, narrow, b3_tiles);
            if (narrow && b3_tiles) cs.fw = Schedule::Fwd();   // (no specialisation carries both: launch by launch, as schedule_get decides)
        } else {
            cs.fw = Schedule::Fwd();
        }
    }
    const std::vector<CensusKernel> kernels = census_kernels();
    const Schedule::Fwd &fw = cs.fw;
    const long long frames = (batch - 1) * window_stride + a->RF;
    const bool shared = call_shares_first_layers(pl, a, batch, uv != 0, window_stride, cam_stride, frames, pl->frame_buf >= 0);
    const int variant = (uv ? 1 : 0) + (shared ? 2 : 0);
    std::vector<GemmProb> rel;
    std::vector<unsigned char> tags;
    const bool has_table = fw.grid > 0 && forward_variant_table(pl, batch, variant, fw.nprob, rel, tags);
    const bool single = !staged && call_is_single(a, b, fw.grid, has_table, fw.kernel, shared);
    CensusOut out{rows, cap};
    // ---- a clip call's launch of per-frame first layers (frame_stage)
    if (shared) {
        std::vector<int4> ft;
        std::vector<int> fo;
        StageSchedule fs{};
        schedule_frame_stage(pl, batch, nwg, ft, fo, fs);
        const char *name = stage_kernel_name(STAGE_BIG, uv != 0, false);
        const CensusKernel *k = census_find(kernels, name);
        if (!k) return -4;
        std::map<std::string, int> hist;
        for (const int4 &t : ft) {
            const Plan::FrameProb &f = pl->frame_probs[t.x & 0xff];
            ++hist[census_tile_kind(*k, CensusProb{false, true, false, false, pl->m[f.model]->layers[f.layer].Kpad}, tile_units(t.x), t.w)];
        }
        out.launch_of(name, fs.nwg, hist);
    }
    if (single) {
        // ---- r3d_bind_f32 (a captured call binds inside its graph; an eager one unless the table is bound to its buffers
        // already - reported here as the first call on them), then the persistent launch (launch_tiles)
        (void)captured;
        out.launch_of(bind_kernel_name(), 1, {});
        const int fwd_kernel = shared ? FWD_KERNEL_CLIP : fw.kernel;
        const char *name = forward_kernel_name(fwd_kernel, uv && fw.uses_gather);
        const CensusKernel *k = census_find(kernels, name);
        if (!k) return -4;
        std::map<std::string, int> hist;
        const int TI = FWD_TILE_INT4 * 4;
        for (int t = 0; t < fw.ntiles; ++t) {
            const int *d = &cs.ft[(size_t)t * TI];
            const int id = d[0] & 0xff;
            ++hist[census_tile_kind(*k, census_prob(&tags[(size_t)id * BIND_NPTR], rel[id].K), tile_units(d[0]), d[3])];
        }
        out.launch_of(name, fw.grid, hist);
    } else {
        // ---- one persistent GEMM launch per level (staged_level)
        CallShape shape;
        shape.uv = uv != 0;
        shape.shared = shared;
        shape.window_stride = window_stride;
        shape.cam_stride = cam_stride;
        shape.frames = frames;
        const Bases none;
        for (size_t si = 0; si < cs.levels->size(); ++si) {
            const auto &st = (*cs.levels)[si];
            const StageSchedule &ss = cs.stages[si];
            std::vector<CensusProb> P(st.size());
            bool uv_launch = false, b3_launch = false;
            for (size_t i = 0; i < st.size(); ++i) {
                GemmProb g;
                unsigned char tg[BIND_NPTR];
                if (fill_prob(pl, pl->probs[st[i] & ~STAGE_SPILL_IN], batch, a, none, shape, g, tg) != R3D_OK) return -3;
                P[i] = census_prob(tg, g.K);
                uv_launch = uv_launch || tg[17] != BIND_NULL;
                b3_launch = b3_launch || P[i].wb3;
            }
            const char *name = stage_kernel_name(ss.kind, uv_launch, b3_launch);
            const CensusKernel *k = census_find(kernels, name);
            if (!k) return -4;
            std::map<std::string, int> hist;
            for (int t = 0; t < ss.ntiles; ++t) {
                const int4 &tl = cs.tiles[ss.tiles_off + t];
                const int slot = tl.x & 0xff;
                if (slot >= (int)st.size()) return -5;
                ++hist[census_tile_kind(*k, P[slot], tile_units(tl.x), tl.w)];
            }
            out.launch_of(name, ss.nwg, hist);
        }
    }
    out.launch_of(decode_kernel_name(batch), 0, {});           // (decoder_tail: its record carries no grid)
    return out.n;
}

int r3d_debug_census_domain(r3d_census_row *rows, int32_t cap) {
    if (!rows && cap > 0) return -1;
    CensusOut out{rows, cap};
    for (const char *name : launch_kernel_names()) out.row(name, 0, "", 0);
    const int codes[] = {1, 2, 4, 8, 16, NB_CODE + 4, NB_CODE + 5, NB_CODE + 6, NB_CODE + 7};
    for (const CensusKernel &k : census_kernels()) {
        std::set<std::string> kinds;
        for (int f = 0; f < 16; ++f)
            for (int K : {64, 96})
                for (int mi = 1; mi <= GEMM_SCHED_MAX_UNITS + 1; ++mi)
                    for (int ks : codes) kinds.insert(census_tile_kind(k, CensusProb{(f & 1) != 0, (f & 2) != 0, (f & 4) != 0, (f & 8) != 0, K}, mi, ks));
        for (const std::string &kind : kinds) out.row(k.name, 0, kind.c_str(), 0);
    }
    return out.n;
}

// Test hook: where the plan kind switches with the window count (r3d_plan.cpp, plan_kind_edges).
int r3d_debug_plan_kind_edges(int64_t *edges, int32_t cap) {
    const std::vector<int64_t> v = plan_kind_edges();
    for (size_t i = 0; i < v.size() && (int32_t)i < cap; ++i)
        if (edges) edges[i] = v[i];
    return (int)v.size();
}

// Test hook: the workspace layout of a call of `batch` windows (include/ray3d_hip.h): the buffers of the plan the driver picks
// (plan_get(plan_kind(batch))) at the offsets fill_prob / frame_stage / decoder_tail give them, then the tail and the control region.
int r3d_debug_plan_buffers(r3d_model *pos, r3d_model *trj, int64_t batch, r3d_plan_buffer_row *rows, int32_t cap, uint64_t *workspace_bytes) {
    const ModelPair mp = model_pair(pos, trj);
    Model *a = mp.a, *b = mp.b;
    if (!a || batch <= 0 || (!rows && cap > 0)) return -1;
    if (b && !same_input_shape(a, b)) return -1;
    const Plan *pl = plan_get(a, b, plan_kind(batch));
    if (!pl) return -2;
    int n = 0;
    auto row = [&](const char *name, int64_t fpw, int per_frame, uint64_t offset, uint64_t bytes) {
        if (n < cap) {
            r3d_plan_buffer_row &r = rows[n];
            memset(&r, 0, sizeof r);
            strncpy(r.name, name, sizeof r.name - 1);
            r.floats_per_window = fpw;
            r.per_frame = per_frame;
            r.offset_bytes = offset;
            r.bytes = bytes;
        }
        ++n;
    };
    for (size_t i = 0; i < pl->buffers.size(); ++i) {
        const BufferSpec &bf = pl->buffers[i];
        if (bf.external != 0) continue;                        // (the caller's camera-parameter rows: no workspace)
        row(bf.name.c_str(), bf.floats_per_window, (int)i == pl->frame_buf ? 1 : 0, (uint64_t)bf.offset_per_window * (uint64_t)batch * sizeof(float),
            (uint64_t)bf.floats_per_window * (uint64_t)batch * sizeof(float));
    }
    const uint64_t used = (uint64_t)pl->floats_per_window * (uint64_t)batch * sizeof(float), act = workspace_act_bytes(pl, batch);
    row("(tail)", pl->tail_floats + 64, 0, used, act - used);
    row("(control)", 0, 0, act, fwd_ctrl_bytes(pl, batch));
    if (workspace_bytes) *workspace_bytes = act + fwd_ctrl_bytes(pl, batch);
    return n;
}

// Test hook: what the forward driver decides from the SHAPE of a call, without a pointer: the size limits (call_size_check,
// px_size_check - check_call and redirect_px ask the same functions) and whether a clip call's first levels read the per-frame
// buffer (call_shares_first_layers, with the tile lists a plan with such a buffer always gets).
int r3d_debug_call_check(r3d_model *pos, r3d_model *trj, int32_t mode, int64_t window_stride, int64_t cam_stride, int64_t batch,
                         int32_t *per_frame) {
    const ModelPair mp = model_pair(pos, trj);
    Model *a = mp.a, *b = mp.b;
    if (per_frame) *per_frame = 0;
    if (!a) { set_error("forward: no model given"); return R3D_ERR_ARG; }
    if (batch <= 0) { set_error("forward: null input/output or B <= 0"); return R3D_ERR_ARG; }
    if (b && !same_input_shape(a, b)) { set_error("pos and trj models disagree on J / F / levels / extrinsic_dim"); return R3D_ERR_ARG; }
    if (mode < R3D_INPUT_RAYS || mode > R3D_INPUT_PX_SCREEN) { set_error("bad input mode %d", mode); return R3D_ERR_ARG; }
    if (window_stride <= 0) { set_error("window_stride must be positive"); return R3D_ERR_ARG; }
    if (const int rc = call_size_check(a, window_stride, batch); rc != R3D_OK) return rc;
    const bool px = mode != R3D_INPUT_RAYS && mode != R3D_INPUT_UV;
    if (px)
        if (const int rc = px_size_check(a, window_stride, cam_stride, batch); rc != R3D_OK) return rc;
    if (per_frame) {
        // (a pixel mode's forward is the R3D_INPUT_RAYS one on what the pre-pass wrote: redirect_px)
        const bool materialised = px && cam_stride != 0 && window_stride < a->RF;
        const int64_t ws = materialised ? a->RF : window_stride;
        const Plan *pl = plan_get(a, b, plan_kind(batch));
        *per_frame = call_shares_first_layers(pl, a, batch, mode == R3D_INPUT_UV, ws, px ? 0 : cam_stride, (batch - 1) * ws + a->RF, pl->frame_buf >= 0) ? 1 : 0;
    }
    return R3D_OK;
}

// Test hook: the pre-pass's per-keypoint routine (r3d_undistort.hpp) on the host.
int r3d_debug_undistort_host(const double *row16, const double *uv, int64_t n, double *out_uv, double *out_rays) {
    if (!row16 || (!uv && n > 0) || n < 0) { set_error("r3d_debug_undistort_host: bad argument"); return R3D_ERR_ARG; }
    const UndistRow k = undist_row(row16);
    for (int64_t i = 0; i < n; ++i) {
        double uo, vo, r[3];
        undistort_pixel(k, uv[2 * i], uv[2 * i + 1], uo, vo);
        pixel_to_ray(k, uo, vo, r);
        if (out_uv) { out_uv[2 * i] = uo; out_uv[2 * i + 1] = vo; }
        if (out_rays) for (int c = 0; c < 3; ++c) out_rays[3 * i + c] = r[c];
    }
    return R3D_OK;
}

// Test hook: the 2-float encodings of the pre-pass (r3d_undistort.hpp) on the host.
int r3d_debug_encode_px_host(const double *row16, const double *uv, int64_t n, int32_t encoding, double *out2) {
    if (!row16 || !out2 || (!uv && n > 0) || n < 0) { set_error("r3d_debug_encode_px_host: bad argument"); return R3D_ERR_ARG; }
    if (encoding != ENC_INTRINSIC && encoding != ENC_SCREEN) {
        set_error("r3d_debug_encode_px_host: encoding must be 1 (intrinsic) or 2 (screen), got %d", encoding);
        return R3D_ERR_ARG;
    }
    for (int64_t i = 0; i < n; ++i) encode_pixel_2d(row16, encoding, uv[2 * i], uv[2 * i + 1], out2 + 2 * i);
    return R3D_OK;
}

// Test hook: r3d_clips_encode on the host - its argument rules (clips_encode_check_args), its descriptor rules and row mapping
// and the pre-pass's per-keypoint routine (r3d_undistort.hpp), clip by clip in table order.
int r3d_debug_clips_encode_host(const float *px, int64_t total_frames, int32_t num_joints, int32_t encoding,
                                const r3d_clip_input_desc *clips, int32_t num_clips, int64_t max_rows, float *x, int64_t out_rows,
                                float *x_mirror, const int32_t *mirror_perm, int32_t *status) {
    const int rc = clips_encode_check_args("r3d_debug_clips_encode_host", px, total_frames, num_joints, encoding, clips, num_clips, max_rows,
                                           x, out_rows, x_mirror, mirror_perm, status);
    if (rc != R3D_OK) return rc;
    unsigned long long inv[2] = {0ull, 0ull};
    if (mirror_perm) mirror_pack_inverse(mirror_perm, num_joints, inv);
    const int J = num_joints, F = enc_floats(encoding);
    for (int32_t c = 0; c < num_clips; ++c) {
        const r3d_clip_input_desc &d = clips[c];
        const bool ok = clip_input_valid(d.first_frame, d.n_frames, d.out_first, d.pad_front, d.pad_back, total_frames, out_rows, max_rows);
        status[c] = ok ? 0 : 1;
        if (!ok) continue;
        const long long rows = d.pad_front + d.n_frames + d.pad_back;
        for (long long r = 0; r < rows; ++r)
            for (int j = 0; j < J; ++j) {
                const long long src = (d.first_frame + clip_input_source(r, d.pad_front, d.n_frames)) * J + j;
                const long long row0 = (d.out_first + r) * J;
                const EncodedPoint pt = encode_point_f32(d.cam, encoding, (double)px[2 * src], (double)px[2 * src + 1]);
                const float e[3] = {pt.x, pt.y, pt.z};
                for (int k = 0; k < F; ++k) x[F * (row0 + j) + k] = e[k];
                if (x_mirror) {
                    float *m = x_mirror + F * (row0 + mirror_dest(inv[0], inv[1], j));
                    for (int k = 0; k < F; ++k) m[k] = k == 0 ? -e[k] : e[k];
                }
            }
    }
    return R3D_OK;
}

// Test hook: the per-frame routines of r3d_clip_valid_losses (r3d_valid.hpp) on the host, frames added in index order.
int r3d_debug_valid_losses_host(const float *pos, const float *trj, const float *gt, int64_t n_frames, int32_t num_joints,
                                const int32_t *parents, int32_t flags, double *out, double *frame) {
    const int rc = valid_check_args("r3d_debug_valid_losses_host", pos, trj, gt, n_frames, num_joints, parents, flags, out);
    if (rc != R3D_OK) return rc;
    ValidIn a;
    a.pos = pos;
    a.trj = trj;
    a.gt = gt;
    a.J = num_joints;
    a.flags = flags;
    a.bones = parents != nullptr;
    a.tree = parents ? valid_pack_tree(parents, num_joints) : ValidTree{{0ull, 0ull}};
    const int nb = a.bones ? num_joints - 1 : 0;
    for (int c = 0; c < R3D_VALID_DOUBLES; ++c) out[c] = 0.0;
    for (int64_t f = 0; f < n_frames; ++f) {
        double term[R3D_VALID_COUNT] = {0, 0, 0, 0, 0, 0, 0};
        valid_frame_terms(a, f, term);
        double bl = 0, bd = 0;
        for (int b = 0; b < nb; ++b) {
            double v[R3D_VALID_BONE_ROWS], dir;
            valid_frame_bone(a, f, b, v, dir);
            bl += v[0];
            bd += dir;
            for (int r = 0; r < R3D_VALID_BONE_ROWS; ++r) out[R3D_VALID_COUNT + r * R3D_VALID_MAX_BONES + b] += v[r];
        }
        if (a.bones) {
            term[R3D_VALID_BONE_LEN] = bl / (double)nb;
            term[R3D_VALID_BONE_DIR] = bd / (double)nb;
        }
        for (int k = 0; k < R3D_VALID_COUNT; ++k) {
            out[k] += term[k];
            if (frame) frame[f * R3D_VALID_COUNT + k] = term[k];
        }
    }
    return R3D_OK;
}

// Test hook: r3d_clips_valid_losses on the host - its argument rules (clips_valid_check_args), its descriptor rule
// (clip_range_valid, the kernels' own) and, per valid clip, r3d_debug_valid_losses_host on the clip's slice, clips in table order.
int r3d_debug_clips_valid_losses_host(const float *pos, const float *trj, const float *gt, int64_t total_frames, int32_t num_joints,
                                      const int32_t *parents, int32_t flags, const r3d_clip_desc *clips, int32_t num_clips,
                                      int64_t max_frames, double *rows, int64_t row_stride, double *frame) {
    const int rc = clips_valid_check_args("r3d_debug_clips_valid_losses_host", pos, trj, gt, total_frames, num_joints, parents, flags, clips,
                                          num_clips, max_frames, rows, row_stride, nullptr, false);
    if (rc != R3D_OK) return rc;
    for (int32_t c = 0; c < num_clips; ++c) {
        const long long first = clips[c].first_frame, n = clips[c].n_frames;
        double *row = rows + (long long)c * row_stride;
        if (!clip_range_valid(first, n, total_frames, max_frames)) {     // not followed: nothing of it is read, its frame rows stay
            for (int k = 0; k < R3D_VALID_DOUBLES; ++k) row[k] = nan("");
            continue;
        }
        const int rc1 = r3d_debug_valid_losses_host(pos + first * num_joints * 3, trj ? trj + first * 3 : nullptr, gt + first * num_joints * 3, n,
                                                    num_joints, parents, flags, row, frame ? frame + first * R3D_VALID_COUNT : nullptr);
        if (rc1 != R3D_OK) return rc1;
    }
    return R3D_OK;
}

// Test hook: r3d_clips_poses on the host - its argument rules (clips_poses_check_args), its descriptor rule (clip_pose_valid) and the
// per-point routines of r3d_poses.hpp, clip by clip in table order.
int r3d_debug_clips_poses_host(const float *raw, const float *raw_mirror, int64_t raw_rows, int32_t num_joints, const int32_t *mirror_perm,
                               const r3d_clip_desc *clips, const int64_t *raw_first, int32_t num_clips, int64_t max_frames,
                               float *pred, double *world, int64_t total_frames, int32_t *status) {
    const int rc = clips_poses_check_args("r3d_debug_clips_poses_host", raw, raw_mirror, raw_rows, num_joints, mirror_perm, clips, raw_first,
                                          num_clips, max_frames, pred, world, total_frames, status);
    if (rc != R3D_OK) return rc;
    unsigned long long perm[2] = {0ull, 0ull};
    if (mirror_perm) pose_pack_perm(mirror_perm, num_joints, perm);
    const int J = num_joints;
    for (int32_t c = 0; c < num_clips; ++c) {
        const long long first = clips[c].first_frame, n = clips[c].n_frames, rf = raw_first[c];
        const bool ok = clip_pose_valid(first, n, rf, total_frames, max_frames, raw_rows);
        status[c] = ok ? 0 : 1;
        if (!ok) continue;
        for (long long f = 0; f < n; ++f)
            for (int j = 0; j < J; ++j) {
                const long long src_row = (rf + f) * J;
                const float *mir = raw_mirror ? raw_mirror + 3 * (src_row + pose_mirror_source(perm[0], perm[1], j)) : nullptr;
                float p[3];
                pose_finish(raw + 3 * (src_row + j), mir, p);
                const long long dst = 3 * ((first + f) * J + j);
                if (pred) memcpy(pred + dst, p, sizeof(p));
                if (world) pose_world(clips[c].rn2w, clips[c].tn2w, p, world + dst);
            }
    }
    return R3D_OK;
}

// Test hook: r3d_clips_project on the host - its argument rules (clips_project_check_args), its descriptor rule (clip_project_valid)
// and the per-point routines of r3d_project.hpp / r3d_undistort.hpp / r3d_poses.hpp, descriptor by descriptor in table order.
int r3d_debug_clips_project_host(const float *world, int64_t total_frames, int32_t num_joints, int32_t encoding,
                                 const r3d_clip_project_desc *clips, int32_t num_clips, int64_t max_rows, float *x, int64_t out_rows,
                                 float *x_mirror, const int32_t *mirror_perm, float *gt, double *px, int64_t gt_rows, int32_t *outside,
                                 int32_t *status) {
    const int rc = clips_project_check_args("r3d_debug_clips_project_host", world, total_frames, num_joints, encoding, clips, num_clips,
                                            max_rows, x, out_rows, x_mirror, mirror_perm, gt, px, gt_rows, status);
    if (rc != R3D_OK) return rc;
    unsigned long long inv[2] = {0ull, 0ull};
    if (mirror_perm) mirror_pack_inverse(mirror_perm, num_joints, inv);
    const int J = num_joints, F = enc_floats(encoding);
    for (int32_t c = 0; c < num_clips; ++c) {
        const r3d_clip_project_desc &d = clips[c];
        const bool ok = clip_project_valid(d.first_frame, d.n_frames, d.out_first, d.pad_front, d.pad_back, d.gt_first, total_frames, out_rows,
                                           max_rows, gt_rows, gt != nullptr || px != nullptr);
        status[c] = ok ? 0 : 1;
        if (!ok) continue;
        const long long rows = d.pad_front + d.n_frames + d.pad_back;
        for (long long r = 0; r < rows; ++r)
            for (int j = 0; j < J; ++j) {
                const float *p = world + 3 * ((d.first_frame + clip_input_source(r, d.pad_front, d.n_frames)) * J + j);
                const long long row0 = (d.out_first + r) * J;
                double u, v;
                project_pixel(d.proj, p, u, v);
                const EncodedPoint pt = encode_point_f32(d.cam, encoding, u, v);
                const float e[3] = {pt.x, pt.y, pt.z};
                for (int k = 0; k < F; ++k) x[F * (row0 + j) + k] = e[k];
                if (x_mirror) {
                    float *m = x_mirror + F * (row0 + mirror_dest(inv[0], inv[1], j));
                    for (int k = 0; k < F; ++k) m[k] = k == 0 ? -e[k] : e[k];
                }
                const long long f = r - d.pad_front;
                if (f < 0 || f >= d.n_frames) continue;          // a padding row: its frame is written by its own row
                const long long at = (d.gt_first + f) * J + j;
                if (gt) {
                    double w[3];
                    pose_world(d.rw2g, d.tw2g, p, w);
                    for (int k = 0; k < 3; ++k) gt[3 * at + k] = encoded_f32(w[k]);
                }
                if (px) {
                    px[2 * at] = pose_f64(u);
                    px[2 * at + 1] = pose_f64(v);
                }
                if (outside && pixel_outside(u, v, d.cam[UNDIST_ROW_RES_W], d.cam[UNDIST_ROW_RES_H])) ++outside[c];
            }
    }
    return R3D_OK;
}

// Test hook: r3d_clips_windows on the host - its argument rules (clips_windows_check_args) and the routines of r3d_windows.hpp the
// kernel's workgroups run: the lookup (bisection, descriptor rule, membership) once per window, then window_point per output point.
int r3d_debug_clips_windows_host(const float *src, int64_t total_frames, int32_t num_joints, int32_t in_features, int32_t receptive_field,
                                 const r3d_window_run_desc *runs, int32_t num_runs, const float *run_param, int32_t extrinsic_dim,
                                 int64_t window0, int64_t batch, float *x, float *param, const int32_t *mirror_perm, int32_t *status) {
    WindowsArgs a;
    const int rc = clips_windows_check_args("r3d_debug_clips_windows_host", src, total_frames, num_joints, in_features, receptive_field, runs,
                                            num_runs, run_param, extrinsic_dim, window0, batch, x, param, mirror_perm, status, &a);
    if (rc != R3D_OK) return rc;
    const long long npts = (long long)a.RF * a.J;
    for (long long w = 0; w < batch; ++w) {
        const WindowRun q = window_lookup(a, w);
        if (!q.ok || q.member) status[q.r] = q.ok ? 0 : 1;
        if (!q.member) continue;
        for (int e = 0; a.param && e < a.E; ++e) a.param[w * a.E + e] = a.run_param[(long long)q.r * a.E + e];
        for (long long pt = 0; pt < npts; ++pt) {
            const int i = (int)(pt / a.J), j = (int)(pt - (long long)i * a.J);
            window_point(a, q.first + window_source_frame(q.start, q.k, q.step, i, q.n), q.flip, j, a.x + a.F * (w * npts + pt));
        }
    }
    return R3D_OK;
}

// Test hook: r3d_streams_step on the host - its argument rules (streams_check_args) and the routines of r3d_streams.hpp the kernel's
// two launches run: every stream advanced (stream_step, stream_store_point, the head, emit and status), then every stream's window
// gathered from what that pass left (stream_emits, stream_gather_point).
int r3d_debug_streams_step_host(void *state, int32_t num_streams, int32_t receptive_field, int32_t lag, int32_t num_joints,
                                int32_t in_features, int32_t encoding, const float *frame, const double *cam, const int32_t *action,
                                float *x, float *x_mirror, const int32_t *mirror_perm, int64_t *emit, int32_t *status) {
    StreamsArgs a;
    const int rc = streams_check_args("r3d_debug_streams_step_host", state, num_streams, receptive_field, lag, num_joints, in_features,
                                      encoding, frame, cam, action, x, x_mirror, mirror_perm, emit, status, &a);
    if (rc != R3D_OK) return rc;
    for (int s = 0; s < a.S; ++s) {
        const StreamStep st = stream_step(a.heads[s].count, a.heads[s].drained, a.action[s], a.lag, a.RF);
        for (int j = 0; st.push && j < a.J; ++j) stream_store_point(a, s, st.slot, j);
        if (st.write_head) {
            a.heads[s].count = st.count;
            a.heads[s].drained = st.drained;
        }
        a.emit[s] = st.emit;
        a.status[s] = st.refused ? 1 : 0;
    }
    for (int s = 0; s < a.S; ++s) {
        const long long c = a.heads[s].count, n = a.emit[s];
        if (!stream_emits(c, a.heads[s].drained, n, a.status[s], a.lag)) continue;
        for (int i = 0; i < a.RF; ++i)
            for (int j = 0; j < a.J; ++j) stream_gather_point(a, s, n, c, i, j);
    }
    return R3D_OK;
}

// Test hook: r3d_streams_poses on the host - its argument rules (streams_poses_check_args), the finished-stream rule and the routines of
// r3d_streams_poses.hpp the kernel runs: per finished stream its J points in joint order, then the quality words from their residuals.
int r3d_debug_streams_poses_host(const float *raw, const float *raw_mirror, int32_t num_streams, int32_t num_joints,
                                 const int32_t *mirror_perm, const int64_t *emit, const int32_t *status, const r3d_stream_pose_desc *desc,
                                 const double *cam, const float *x, int32_t receptive_field, int32_t lag, float *pred, double *world,
                                 double *reproj, double *quality) {
    StreamsPosesArgs a;
    const int rc = streams_poses_check_args("r3d_debug_streams_poses_host", raw, raw_mirror, num_streams, num_joints, mirror_perm, emit,
                                            status, desc, cam, x, receptive_field, lag, pred, world, reproj, quality, &a);
    if (rc != R3D_OK) return rc;
    for (int s = 0; s < a.S; ++s) {
        if (!stream_finished(a.status[s], a.emit[s])) continue;
        double res[17];
        for (int j = 0; j < a.J; ++j) res[j] = stream_pose_point(a, s, j);
        if (a.quality) stream_quality(res, a.J, a.quality + 2 * s);
    }
    return R3D_OK;
}

// Test hook: r3d_streams_repair on the host - its argument rules (streams_repair_check_args) and the routines of r3d_streams_repair.hpp
// the kernel runs: per stream the verdict on the head and the action word, then - for a stream that takes a push - the track zeroed
// on a RESTART, its J joints in joint order, and the two mask words from the joints that were not observed.
int r3d_debug_streams_repair_host(void *state, void *track, int32_t num_streams, int32_t receptive_field, int32_t lag,
                                  int32_t num_joints, int32_t in_features, int32_t encoding, const float *frame, const float *conf,
                                  float min_conf, const double *cam, const int32_t *action, int32_t max_gap, float *frame_out,
                                  uint32_t *synthetic) {
    StreamsRepairArgs a;
    const int rc = streams_repair_check_args("r3d_debug_streams_repair_host", state, track, num_streams, receptive_field, lag, num_joints,
                                             in_features, encoding, frame, conf, min_conf, cam, action, max_gap, frame_out, synthetic, &a);
    if (rc != R3D_OK) return rc;
    for (int s = 0; s < a.S; ++s) {
        const StreamRepairStep rs = stream_repair_step(a, s);
        if (!rs.st.push) {
            a.synthetic[s] = stream_repair_idle_word(a, s, rs.st);
            continue;
        }
        for (int i = 0; rs.restart && i < stream_repair_track_words(a); ++i) stream_repair_zero(a, s, i);
        uint32_t mask = 0;
        for (int j = 0; j < a.J; ++j)
            if (stream_repair_joint(a, s, j, rs.c, rs.restart)) mask |= 1u << j;
        stream_repair_finish(a, s, rs.c, mask);
    }
    return R3D_OK;
}

// Test hook: r3d_clips_repair on the host - its argument rules (clips_repair_check_args) and the routines of r3d_clips_repair.hpp the
// kernel runs: per clip the verdict on the descriptor, then per joint the bitmap of observed rows built from the contents at entry
// and, in the kernel's steps of 256 rows with its carry, every missing point through clip_repair_point.
int r3d_debug_clips_repair_host(float *x, int64_t out_rows, int32_t num_joints, int32_t in_features, float *x_mirror,
                                const int32_t *mirror_perm, const r3d_clip_input_desc *clips, int32_t num_clips, int64_t max_rows,
                                const float *conf, int64_t total_frames, float min_conf, int32_t max_gap, uint8_t *state, int32_t *stats,
                                int32_t *status) {
    ClipsRepairArgs a;
    const int rc = clips_repair_check_args("r3d_debug_clips_repair_host", x, out_rows, num_joints, in_features, x_mirror, mirror_perm, clips,
                                           num_clips, max_rows, conf, total_frames, min_conf, max_gap, state, stats, status, &a);
    if (rc != R3D_OK) return rc;
    std::vector<unsigned long long> bits(CLIPS_REPAIR_WORDS);
    for (int32_t ci = 0; ci < num_clips; ++ci) {
        const ClipRepairClip c = clip_repair_clip(a, clips + ci);
        status[ci] = c.ok ? 0 : 1;
        if (!c.ok) continue;
        const int steps = (c.R + CLIPS_REPAIR_THREADS - 1) / CLIPS_REPAIR_THREADS;
        for (int j = 0; j < a.J; ++j) {
            int first = -1;
            for (int w = 0; w < steps * CLIPS_REPAIR_WAVES; ++w) bits[w] = 0ull;
            for (int r = 0; r < c.R; ++r)
                if (clip_repair_observed(a, c, r, j)) {
                    bits[r >> 6] |= 1ull << (r & 63);
                    if (first < 0) first = r;
                }
            int carry = -1, cnt[5] = {0, 0, 0, 0, 0};
            for (int base = 0; base < c.R; base += CLIPS_REPAIR_THREADS) {
                for (int r = base; r < c.R && r < base + CLIPS_REPAIR_THREADS; ++r) {
                    int st = CLIP_REPAIR_OBSERVED;
                    if (!((bits[r >> 6] >> (r & 63)) & 1ull)) st = clip_repair_point(a, c, bits.data(), first, clip_repair_prev(bits.data(), r, carry), r, j);
                    if (state) state[(c.out_first + r) * a.J + j] = (uint8_t)st;
                    if (r >= c.pad_front && r < c.pad_front + c.n) ++cnt[st];
                }
                carry = clip_repair_carry(bits.data(), base >> 6, carry);
            }
            for (int k = 0; stats && k < 4; ++k) stats[((long long)ci * a.J + j) * 4 + k] = cnt[k + 1];
        }
    }
    return R3D_OK;
}

// Test hook: r3d_streams_peek on the host - its argument rules (streams_peek_check_args) and the routines of r3d_streams_peek.hpp the
// kernel runs: per look and stream the verdict (stream_peek) and its two words, then - for a stream that previews - the window's
// points in row and joint order (stream_peek_point).
int r3d_debug_streams_peek_host(const void *state, int32_t num_streams, int32_t receptive_field, int32_t lag, int32_t num_joints,
                                int32_t in_features, const int32_t *looks, int32_t num_looks, const int32_t *action, const int32_t *status,
                                float *x, float *x_mirror, const int32_t *mirror_perm, int64_t *emit, int32_t *peek_status) {
    StreamsPeekArgs a;
    const int rc = streams_peek_check_args("r3d_debug_streams_peek_host", state, num_streams, receptive_field, lag, num_joints, in_features,
                                           looks, num_looks, action, status, x, x_mirror, mirror_perm, emit, peek_status, &a);
    if (rc != R3D_OK) return rc;
    for (int k = 0; k < a.K; ++k)
        for (int s = 0; s < a.S; ++s) {
            const long long c = a.heads[s].count;
            const StreamPeek pk = stream_peek(c, a.heads[s].drained, a.action != nullptr, a.action ? a.action[s] : R3D_STREAM_PUSH,
                                              a.status[s], stream_peek_look(a, k), a.lag);
            a.emit[(long long)k * a.S + s] = pk.p;
            a.peek_status[(long long)k * a.S + s] = pk.bad ? 1 : 0;
            if (!pk.previews) continue;
            for (int i = 0; i < a.RF; ++i)
                for (int j = 0; j < a.J; ++j) stream_peek_point(a, k, s, pk.p, c, i, j);
        }
    return R3D_OK;
}

// Test hook: r3d_streams_fuse on the host - its argument rules (streams_fuse_check_args) and the routine of r3d_streams_fuse.hpp the
// kernel runs: per group its J joints in joint order through stream_fuse_joint on a staging area of stride 1, then the `used` words
// from the joints' inlier masks, as the wavefront's ballots form them.
int r3d_debug_streams_fuse_host(const double *world, const double *reproj, const int64_t *emit, const int32_t *status,
                                const uint32_t *synthetic, int32_t num_streams, int32_t num_joints, const int32_t *member,
                                int32_t num_groups, int32_t max_members, double soft_px, double max_px, double max_dist, double *fused,
                                double *spread, int32_t *count, uint32_t *used) {
    StreamsFuseArgs a;
    const int rc = streams_fuse_check_args("r3d_debug_streams_fuse_host", world, reproj, emit, status, synthetic, num_streams, num_joints,
                                           member, num_groups, max_members, soft_px, max_px, max_dist, fused, spread, count, used, &a);
    if (rc != R3D_OK) return rc;
    for (int g = 0; g < a.G; ++g) {
        uint32_t words[R3D_FUSE_MAX_MEMBERS] = {};
        for (int j = 0; j < a.J; ++j) {
            double stage[STREAMS_FUSE_STAGE];
            const uint32_t inl = stream_fuse_joint(a, g, j, stage, 1);
            for (int m = 0; m < a.M; ++m) words[m] |= ((inl >> m) & 1u) << j;
        }
        for (int m = 0; a.used && m < a.M; ++m) a.used[(long long)g * a.M + m] = words[m];
    }
    return R3D_OK;
}

// Test hook: r3d_streams_assign on the host - its argument rules (streams_assign_check_args) and the routines of
// r3d_streams_assign.hpp the kernel runs: per camera the detections' summaries, the P x D cost keys, the greedy matching as plain
// loops over the same keys in the kernel's order (stream_assign_better), the free-slot and leftover masks the kernel forms with
// ballots, then the slots in order and the camera's finish.
int r3d_debug_streams_assign_host(void *assign, const r3d_assign_params *prm, const float *det, const float *det_conf,
                                  const int32_t *det_count, int32_t *action, float *frame_out, float *conf_out, int32_t *match,
                                  int64_t *id, int32_t *stats) {
    StreamsAssignArgs a;
    const int rc = streams_assign_check_args("r3d_debug_streams_assign_host", assign, prm, det, det_conf, det_count, action, frame_out,
                                             conf_out, match, id, stats, &a);
    if (rc != R3D_OK) return rc;
    const StreamAssignState st = stream_assign_state(a);
    unsigned long long key[R3D_ASSIGN_MAX_SLOTS * R3D_ASSIGN_MAX_DETECTIONS];      // [p * D + d]
    for (int c = 0; c < a.C; ++c) {
        const int n = stream_assign_count(a.det_count[c], a.D);
        StreamAssignDet dets[R3D_ASSIGN_MAX_DETECTIONS];
        uint32_t valid = 0;
        for (int d = 0; d < a.D; ++d) {
            dets[d] = d < n ? stream_assign_detection(a, c, d) : StreamAssignDet{0u, 0.0, false};
            if (dets[d].valid) valid |= 1u << d;
        }
        for (int p = 0; p < a.P; ++p)
            for (int d = 0; d < a.D; ++d) key[p * a.D + d] = stream_assign_pair(a, st, c, p, d, dets[d]);
        uint32_t rows = 0, cols = 0, free_mask = 0;
        int matched[R3D_ASSIGN_MAX_SLOTS];
        for (int p = 0; p < a.P; ++p) matched[p] = -1;
        for (;;) {
            unsigned long long best = STREAM_ASSIGN_NONE;
            int at = a.P * a.D;
            for (int i = 0; i < a.P * a.D; ++i) {
                const int p = i / a.D, d = i - p * a.D;
                if (((rows >> p) | (cols >> d)) & 1u) continue;
                if (stream_assign_better(key[i], i, best, at)) {
                    best = key[i];
                    at = i;
                }
            }
            if (best == STREAM_ASSIGN_NONE) break;
            const int p = at / a.D, d = at - p * a.D;
            rows |= 1u << p;
            cols |= 1u << d;
            matched[p] = d;
        }
        for (int p = 0; p < a.P; ++p)
            if (stream_assign_phase(st.phase[(long long)c * a.P + p], a.lag) == 0) free_mask |= 1u << p;
        const uint32_t unmatched = valid & ~cols;
        const long long next = st.next_id[c];
        for (int p = 0; p < a.P; ++p) stream_assign_slot(a, st, c, p, matched[p], free_mask, unmatched, next);
        stream_assign_finish(a, st, c, valid, cols, free_mask, unmatched, next);
    }
    return R3D_OK;
}

// Test hook: r3d_streams_link on the host - its argument rules (streams_link_check_args) and the routines of r3d_streams_link.hpp
// the kernel runs: per scene and camera the links' tests in ascending g (a stream a smaller g holds is dropped), the slots'
// summaries, the G x P cost keys, the greedy matching as plain loops over the same keys in the kernel's order
// (stream_assign_better), the births by the ranks the kernel forms with ballots, then the people in order and the scene's finish.
int r3d_debug_streams_link_host(void *link, const r3d_link_params *prm, const double *world, const int64_t *emit, const int32_t *status,
                                const int64_t *id, int32_t *member, int64_t *person, int32_t *group, int32_t *stats) {
    StreamsLinkArgs a;
    const int rc = streams_link_check_args("r3d_debug_streams_link_host", link, prm, world, emit, status, id, member, person, group, stats, &a);
    if (rc != R3D_OK) return rc;
    const StreamLinkState st = stream_link_state(a);
    unsigned long long key[R3D_LINK_MAX_PEOPLE * R3D_ASSIGN_MAX_SLOTS];            // [g * P + p]
    for (int n = 0; n < a.N; ++n) {
        bool entry[R3D_LINK_MAX_PEOPLE], alive[R3D_LINK_MAX_PEOPLE];
        for (int g = 0; g < a.G; ++g) {
            entry[g] = alive[g] = st.phase[n * a.G + g] == 1;
        }
        long long next = st.next_id[n];
        int links = 0, births = 0, dropped = 0;
        for (int c = 0; c < a.C; ++c) {
            int p1[R3D_LINK_MAX_PEOPLE];
            bool made[R3D_LINK_MAX_PEOPLE];
            uint32_t held = 0, cand = 0, elig = 0, free_mask = 0, pres[R3D_ASSIGN_MAX_SLOTS];
            for (int g = 0; g < a.G; ++g) {
                made[g] = false;
                p1[g] = entry[g] ? stream_link_validate(a, st, n, (uint32_t)(n * a.G + g), c) : 0;
                if (p1[g] == 0) continue;
                if ((held >> (p1[g] - 1)) & 1u) p1[g] = 0;          // a smaller g holds the stream
                else held |= 1u << (p1[g] - 1);
            }
            for (int p = 0; p < a.P; ++p)
                if (stream_link_candidate(a, n, c, p, held, &pres[p])) cand |= 1u << p;
            for (int g = 0; g < a.G; ++g)
                if (alive[g] && p1[g] == 0 && stream_link_seen(st.seen[n * a.G + g], a.J) != 0u) elig |= 1u << g;
            uint32_t rows = 0, cols = 0;
            if (cand && elig) {
                for (int g = 0; g < a.G; ++g)
                    for (int p = 0; p < a.P; ++p)
                        key[g * a.P + p] = ((cand >> p) & (elig >> g) & 1u) ? stream_link_pair(a, st, n, g, c, p, pres[p]) : STREAM_ASSIGN_NONE;
                for (;;) {
                    unsigned long long best = STREAM_ASSIGN_NONE;
                    int at = a.G * a.P;
                    for (int i = 0; i < a.G * a.P; ++i) {
                        const int g = i / a.P, p = i - g * a.P;
                        if (((rows >> g) | (cols >> p)) & 1u) continue;
                        if (stream_assign_better(key[i], i, best, at)) {
                            best = key[i];
                            at = i;
                        }
                    }
                    if (best == STREAM_ASSIGN_NONE) break;
                    const int g = at / a.P, p = at - g * a.P;
                    rows |= 1u << g;
                    cols |= 1u << p;
                    p1[g] = p + 1;
                    made[g] = true;
                }
            }
            const uint32_t unmatched = cand & ~cols;
            for (int g = 0; g < a.G; ++g)
                if (!alive[g]) free_mask |= 1u << g;
            const int want = __builtin_popcount(unmatched), room = __builtin_popcount(free_mask);
            const int born = want < room ? want : room;
            for (int g = 0; g < a.G; ++g) {
                if (!((free_mask >> g) & 1u)) continue;
                const int rank = __builtin_popcount(free_mask & ((1u << g) - 1u));
                if (rank >= want) continue;
                const int p = stream_assign_nth_bit(unmatched, rank);
                stream_link_birth(a, st, (uint32_t)(n * a.G + g), stream_link_stream(a, n, c, p),
                                            (long long)((unsigned long long)next + (unsigned long long)rank));
                alive[g] = true;
                p1[g] = p + 1;
                made[g] = true;
            }
            next = (long long)((unsigned long long)next + (unsigned long long)born);
            links += __builtin_popcount(cols);
            births += born;
            dropped += want - born;
            for (int g = 0; g < a.G; ++g) stream_link_store(a, st, n, (uint32_t)(n * a.G + g), c, p1[g], made[g]);
            if (a.group)
                for (int p = 0; p < a.P; ++p) {
                    int32_t who = -1;
                    for (int g = a.G - 1; g >= 0; --g)
                        if (p1[g] == p + 1) who = n * a.G + g;
                    a.group[stream_link_stream(a, n, c, p)] = who;
                }
        }
        int lives = 0;
        for (int g = 0; g < a.G; ++g) {
            const uint32_t gi = (uint32_t)(n * a.G + g);
            int32_t tbl[R3D_FUSE_MAX_MEMBERS];
            uint32_t add = 0;
            const bool linked = alive[g] && stream_link_members(a, st, n, gi, tbl);
            if (alive[g])
                for (int j = 0; j < a.J; ++j)
                    if (stream_link_joint(a, st, gi, j, tbl)) add |= 1u << j;
            lives += stream_link_person(a, st, gi, alive[g], linked, add) ? 1 : 0;
        }
        st.next_id[n] = next;
        if (a.stats) {
            a.stats[4 * n] = lives;
            a.stats[4 * n + 1] = links;
            a.stats[4 * n + 2] = births;
            a.stats[4 * n + 3] = dropped;
        }
    }
    return R3D_OK;
}

// Test hook: the tables and per-element routines of r3d_finalize_dev against model_pack_host, on the CPU (r3d_model.cpp)
int r3d_debug_pack_replay_host(r3d_model *m, int64_t *mismatches, int64_t *first_index) {
    return model_pack_replay_host(reinterpret_cast<Model *>(m), mismatches, first_index);
}

// Test hook: the packed image as the device holds it (the one device call of this file: tests compare the two finalize paths' bytes)
int r3d_debug_weights_image(r3d_model *m, float *out, size_t cap_floats, size_t *need_floats) {
    Model *mm = reinterpret_cast<Model *>(m);
    if (!mm || !need_floats) { set_error("r3d_debug_weights_image: null argument"); return R3D_ERR_ARG; }
    if (!mm->finalized || !mm->d_arena) { set_error("r3d_debug_weights_image: the handle is not finalized"); return R3D_ERR_STATE; }
    *need_floats = mm->arena_floats;
    if (!out || cap_floats < mm->arena_floats) { set_error("r3d_debug_weights_image: %zu floats are needed", mm->arena_floats); return R3D_ERR_WORKSPACE; }
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "hipDeviceSynchronize");
    if ((e = hipMemcpy(out, mm->d_arena, mm->arena_floats * sizeof(float), hipMemcpyDeviceToHost)) != hipSuccess) return hip_fail(e, "hipMemcpy(image)");
    return R3D_OK;
}

}  // extern "C"

#endif  // R3D_TEST_HOOKS
