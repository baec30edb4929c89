// R3D_TIMING builds (make timing, tools/build_probe.sh): the phase stamps of a launch - "arm" hands the kernel a zeroed stamp
// buffer ahead of the launch, "report" waits for the launch and prints / dumps what it stamped.  tools/fwd_gantt.py and
// tools/stage_times.py parse the output.
#ifdef R3D_TIMING
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "r3d_internal.hpp"

namespace r3d {

static long long *timing_buf1 = nullptr;   // the single-launch forward

void timing_arm_forward(const Schedule::Fwd &fw, FwdArgs &fa, hipStream_t stream) {
    if (getenv("R3D_TIMING_STAGE")) {
        const size_t tbytes = (16384 + 4 * 65536) * 8;
        if (!timing_buf1) (void)hipMalloc((void **)&timing_buf1, tbytes);
        (void)hipMemsetAsync(timing_buf1, 0, tbytes, stream);
        if (fw.ntiles <= 65536) fa.dbg = timing_buf1;
    }
}

void timing_report_forward(const Plan *pl, const Schedule::Fwd &fw, const FwdArgs &fa, int64_t B, hipStream_t stream) {
    if (fa.dbg) {
        (void)hipStreamSynchronize(stream);
        std::vector<long long> hw(4 * 1024);
        (void)hipMemcpy(hw.data(), timing_buf1 + 1024, hw.size() * 8, hipMemcpyDeviceToHost);
        long long w0 = 1LL << 62, w1 = 0, e0 = 1LL << 62;
        std::vector<double> d;
        for (int w = 0; w < fw.grid && w < 1024; ++w) {
            w0 = std::min(w0, hw[w * 4 + 2]); w1 = std::max(w1, hw[w * 4 + 3]); e0 = std::min(e0, hw[w * 4 + 3]);
            d.push_back((hw[w * 4 + 3] - hw[w * 4 + 2]) / 100.0);
        }
        std::sort(d.begin(), d.end());
        fprintf(stderr, "[timing] forward: first workgroup start -> last end %.2f us; ends spread over %.2f us; busy min %.1f median %.1f max %.1f us\n",
                (w1 - w0) / 100.0, (w1 - e0) / 100.0, d.front(), d[d.size() / 2], d.back());
        if (getenv("R3D_TIMING_ALL"))
            for (int w = 0; w < fw.grid && w < 1024; ++w)
                fprintf(stderr, "[timing-wg] %d start %.2f end %.2f\n", w, (hw[w * 4 + 2] - w0) / 100.0, (hw[w * 4 + 3] - w0) / 100.0);
        if (const char *dump = getenv("R3D_TIMING_DUMP")) {      // every tile: who ran it, what it is, fetched / ready / finished
            std::vector<long long> tt((size_t)fw.ntiles * 4);
            (void)hipMemcpy(tt.data(), timing_buf1 + 16384, tt.size() * 8, hipMemcpyDeviceToHost);
            if (FILE *f = fopen(dump, "w")) {
                for (int i = 0; i < fw.nprob; ++i) {
                    const ProbSpec &q = pl->probs[i];
                    fprintf(f, "P %d %s rows_per_window %d M %lld N %d K %d fused %d\n", i, pl->m[q.model]->layers[q.layer].weight_key.c_str(),
                            q.rows_per_window, (long long)(B * q.rows_per_window), pl->m[q.model]->layers[q.layer].N,
                            pl->m[q.model]->layers[q.layer].Kpad, q.layer3 >= 0 ? 3 : q.layer2 >= 0 ? 2 : 1);
                }
                for (int w = 0; w < fw.grid; ++w)
                    for (int t = fw.h_wgoff[w]; t < fw.h_wgoff[w + 1]; ++t) {
                        const int *d = &fw.h_tiles[(size_t)t * FWD_TILE_INT4 * 4];
                        fprintf(f, "T %d %d %d %d %d %d %d %d %.2f %.2f %.2f %lld %d\n", w, t, d[0] & 0xff, tile_units(d[0]), d[1], d[2], d[3], d[4],
                                tt[(size_t)t * 4] ? (tt[(size_t)t * 4] - w0) / 100.0 : -1.0, tt[(size_t)t * 4 + 1] ? (tt[(size_t)t * 4 + 1] - w0) / 100.0 : -1.0,
                                tt[(size_t)t * 4 + 2] ? (tt[(size_t)t * 4 + 2] - w0) / 100.0 : -1.0, tt[(size_t)t * 4 + 3],
                                tile_src2(d[0]));      // (last: a two-source tile's second problem, or -1)
                    }
                fclose(f);
            }
        }
    }
}

// development build only (tools/build_probe.sh): phase stamps of the first tiles of launch $R3D_TIMING_STAGE
static long long *timing_buf = nullptr;

bool timing_arm_stage(size_t si, LaunchArgs &la, hipStream_t stream) {
    const char *tstage = getenv("R3D_TIMING_STAGE");
    const bool timed = tstage && (!strcmp(tstage, "all") || atoi(tstage) == (int)si);
    if (timed) {
        if (!timing_buf) (void)hipMalloc((void **)&timing_buf, (1024 + 4 * 1024) * 8 + 65536);
        (void)hipMemsetAsync(timing_buf, 0, (1024 + 4 * 1024) * 8 + 65536, stream);
        la.dbg = timing_buf;
    }
    return timed;
}

void timing_report_stage(size_t si, const StageSchedule &ss, hipStream_t stream) {
    (void)hipStreamSynchronize(stream);
    std::vector<long long> ht(16 * 64);
    (void)hipMemcpy(ht.data(), timing_buf + 6144, ht.size() * 8, hipMemcpyDeviceToHost);
    std::vector<long long> hw(4 * 1024);
    (void)hipMemcpy(hw.data(), timing_buf + 1024, hw.size() * 8, hipMemcpyDeviceToHost);
    long long w0 = 1LL << 62, w1 = 0, s1 = 0, e0 = 1LL << 62;
    for (int w = 0; w < ss.nwg && w < 1024; ++w) {
        w0 = std::min(w0, hw[w * 4 + 2]); s1 = std::max(s1, hw[w * 4 + 2]);
        w1 = std::max(w1, hw[w * 4 + 3]); e0 = std::min(e0, hw[w * 4 + 3]);
    }
    fprintf(stderr, "[timing] launch %zu: first workgroup start -> last end %.2f us; starts spread over %.2f us, ends over %.2f us; "
            "wg 0: start -> first tile entry %.2f us\n", si, (w1 - w0) / 100.0, (s1 - w0) / 100.0, (w1 - e0) / 100.0,
            (ht[0] - hw[2]) / 100.0);
    {   // distribution of the workgroups' busy times (start -> end of the persistent loop)
        std::vector<double> d;
        for (int w = 0; w < ss.nwg && w < 1024; ++w) d.push_back((hw[w * 4 + 3] - hw[w * 4 + 2]) / 100.0);
        std::sort(d.begin(), d.end());
        if (!d.empty())
            fprintf(stderr, "[timing] launch %zu: workgroup busy time min %.1f  p10 %.1f  median %.1f  p90 %.1f  max %.1f us (%zu workgroups)\n", si,
                    d.front(), d[d.size() / 10], d[d.size() / 2], d[d.size() * 9 / 10], d.back(), d.size());
        {   // shader clock during the launch: cycle counter against the 100 MHz wall clock, median over the workgroups
            std::vector<double> g;
            for (int w = 0; w < ss.nwg && w < 1024; ++w)
                if (hw[w * 4 + 3] > hw[w * 4 + 2]) g.push_back((double)(hw[w * 4 + 1] - hw[w * 4 + 0]) / ((hw[w * 4 + 3] - hw[w * 4 + 2]) * 10.0));
            std::sort(g.begin(), g.end());
            if (!g.empty()) fprintf(stderr, "[timing] launch %zu: shader clock %.2f GHz (median), %.2f .. %.2f\n", si, g[g.size() / 2], g.front(), g.back());
        }
        if (getenv("R3D_TIMING_ALL"))
            for (int w = 0; w < ss.nwg && w < 1024; ++w)
                fprintf(stderr, "[timing-wg] %d start %.2f end %.2f\n", w, (hw[w * 4 + 2] - w0) / 100.0, (hw[w * 4 + 3] - w0) / 100.0);
    }
    fprintf(stderr, "[timing] launch %zu: wg tile | phase lengths in us (100 MHz wall clock)\n", si);
    for (int w = 0; w < 16 && w < ss.nwg; ++w)
        for (int t = 0; t < 8; ++t) {
            const long long *q = &ht[w * 64 + t * 8];
            if (!q[0]) continue;
            fprintf(stderr, "  wg %2d tile %d: %6.2f %6.2f %6.2f %6.2f | total %6.2f", w, t, (q[1] - q[0]) / 100.0,
                    (q[2] - q[1]) / 100.0, (q[3] - q[2]) / 100.0, (q[4] - q[3]) / 100.0, (q[4] - q[0]) / 100.0);
            if (q[5]) fprintf(stderr, " | first tap: expand %6.2f  H write %6.2f  3-tap third %6.2f", (q[5] - q[0]) / 100.0,
                              (q[6] - q[5]) / 100.0, (q[7] - q[6]) / 100.0);
            fprintf(stderr, "\n");
        }
}

}  // namespace r3d

#endif  // R3D_TIMING
