// The process-wide ordering of single-launch forwards, and the R3D_OPT_LANES streams that take part in it.
#include <algorithm>
#include <mutex>

#include "r3d_internal.hpp"

namespace r3d {

// Two single-launch forwards must never be on the GPU at the same time: each needs ALL its workgroups resident (a waiting
// workgroup spins for tiles of workgroups that may not have been dispatched yet), and two such kernels from two streams
// could each hold part of the chip and wait for the rest forever (until the bounded spins give up).  Within a process the
// library therefore orders them: per device it remembers the stream and an event of the last single-launch forward, and a
// forward on ANOTHER stream first records an event behind the work of the previous forward's stream and waits for it (a
// device-side dependency, no host synchronisation).  The common case - one stream - costs a mutex and a compare.  Streams being captured are left alone (a capture
// must not wait on events from outside it): capture one forward stream per graph, replay graphs one at a time.
struct FwdOrder {
    std::mutex mu;
    hipEvent_t ev[64] = {nullptr};
    hipStream_t last[64] = {nullptr};
    bool have[64] = {false};
    // R3D_OPT_CU_LIMIT: forwards on CU-masked streams are not ordered against EACH OTHER (disjoint masks: that is their point), but
    // a whole-device forward and a masked one must never share the chip either: the streams that have run a masked forward since
    // the last whole-device forward waited for them
    std::vector<hipStream_t> masked[64];
    // ... and a masked stream waits behind the last whole-device forward ONCE, not with every call: `gen` counts the device's
    // whole-device forwards, `seen` which one each masked stream has waited for.  (An event per call would be recorded on the
    // whole-device forward's stream - usually the legacy default stream, where an event is behind the work of EVERY blocking
    // stream, the other lanes' forwards in flight included: the masked streams would run one after the other.)
    struct Seen { hipStream_t s; unsigned long long gen; };
    std::vector<Seen> seen[64];
    unsigned long long gen[64] = {0};
};
static FwdOrder g_fwd_order;
std::mutex g_fwd_launch_mu;             // order_single_launch(before) .. launch .. order_single_launch(after) of one forward

// A stream of the library's own is about to be destroyed: nothing may record events on it any more.
static void order_forget(hipStream_t stream) {
    std::lock_guard<std::mutex> lock(g_fwd_order.mu);
    FwdOrder &o = g_fwd_order;
    for (int d = 0; d < 64; ++d) {
        o.masked[d].erase(std::remove(o.masked[d].begin(), o.masked[d].end(), stream), o.masked[d].end());
        o.seen[d].erase(std::remove_if(o.seen[d].begin(), o.seen[d].end(), [&](const FwdOrder::Seen &x) { return x.s == stream; }), o.seen[d].end());
        if (o.have[d] && o.last[d] == stream) o.have[d] = false;
    }
}

// `behind`: make `stream` wait (device-side) for everything `other` has been given so far.  A stream that is gone or capturing is skipped.
hipError_t wait_behind(hipStream_t stream, hipStream_t other, hipEvent_t &ev) {
    if (other == stream) return hipSuccess;
    if (other == nullptr) {          // the legacy default stream: a blocking stream is behind its work already (and an event on it would be
        unsigned flags = 0;          // behind every other blocking stream's work too - see FwdOrder::seen)
        if (hipStreamGetFlags(stream, &flags) == hipSuccess && !(flags & hipStreamNonBlocking)) return hipSuccess;
        (void)hipGetLastError();
    }
    hipStreamCaptureStatus ocs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(other, &ocs) != hipSuccess || ocs != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return hipSuccess; }
    if (!ev) {
        hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e != hipSuccess) return e;
    }
    hipError_t e = hipEventRecord(ev, other);
    if (e != hipSuccess) { (void)hipGetLastError(); return hipSuccess; }      // (the other stream is gone: nothing of it can still run)
    return hipStreamWaitEvent(stream, ev, 0);
}

// masked: the forward runs on a CU-masked stream with R3D_OPT_CU_LIMIT workgroups.  Rules: whole-device forwards are ordered among
// themselves and behind every masked forward issued before them; a masked forward is ordered behind the last whole-device forward;
// masked forwards of different streams are not ordered against each other.
hipError_t order_single_launch(hipStream_t stream, bool before, bool masked) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipSuccess;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) != hipSuccess) { (void)hipGetLastError(); return hipSuccess; }
    if (cs != hipStreamCaptureStatusNone) return hipSuccess;
    std::lock_guard<std::mutex> lock(g_fwd_order.mu);
    FwdOrder &o = g_fwd_order;
    if (!before) {                                   // (after the launch: just remember whose it was - no event on the one-stream path)
        if (masked) {
            if (std::find(o.masked[dev].begin(), o.masked[dev].end(), stream) == o.masked[dev].end()) o.masked[dev].push_back(stream);
        } else {
            o.last[dev] = stream;
            o.have[dev] = true;
            ++o.gen[dev];
        }
        return hipSuccess;
    }
    // another stream ran the previous whole-device forward: an event behind everything that stream has been given so far, and wait for it
    if (o.have[dev] && o.last[dev] != stream) {
        bool wait = true;
        if (masked) {                                // (once per whole-device forward and masked stream)
            auto it = std::find_if(o.seen[dev].begin(), o.seen[dev].end(), [&](const FwdOrder::Seen &x) { return x.s == stream; });
            if (it == o.seen[dev].end()) o.seen[dev].push_back({stream, o.gen[dev]});
            else if (it->gen == o.gen[dev]) wait = false;
            else it->gen = o.gen[dev];
        }
        if (wait)
            if (hipError_t e = wait_behind(stream, o.last[dev], o.ev[dev]); e != hipSuccess) return e;
    }
    if (!masked) {
        for (hipStream_t ms : o.masked[dev])
            if (hipError_t e = wait_behind(stream, ms, o.ev[dev]); e != hipSuccess) return e;
        o.masked[dev].clear();                       // (they re-enter the list with their next masked forward)
    }
    return hipSuccess;
}

// CU mask of lane k of n: CUs c of every XCD with c % n == k (mask bit i is CU i / 8 of XCD i % 8: consecutive bits go to consecutive
// XCDs) - every lane spans all eight XCDs and their L2s with device CUs / n CUs
int lanes_create(Model *m, int n) {
    const int cus = device_cu_count();
    const int words = (cus + 31) / 32;
    for (int k = 0; k < n; ++k) {
        std::vector<uint32_t> mask((size_t)std::max(words, 1), 0u);
        for (int i = 0; i < cus; ++i)
            if ((i / 8) % n == k) mask[(size_t)i / 32] |= 1u << (i % 32);
        hipError_t e = hipExtStreamCreateWithCUMask(&m->lane[k].stream, (uint32_t)mask.size(), mask.data());
        if (e != hipSuccess) return hip_fail(e, "hipExtStreamCreateWithCUMask");
        if ((e = hipEventCreateWithFlags(&m->lane[k].done, hipEventDisableTiming)) != hipSuccess) return hip_fail(e, "hipEventCreate");
        if ((e = hipEventCreateWithFlags(&m->lane[k].in, hipEventDisableTiming)) != hipSuccess) return hip_fail(e, "hipEventCreate");
    }
    return R3D_OK;
}
void lanes_destroy(Model *m) {
    for (auto &ln : m->lane) {
        if (ln.done) (void)hipEventDestroy(ln.done);
        if (ln.in) (void)hipEventDestroy(ln.in);
        if (ln.stream) {
            order_forget(ln.stream);
            (void)hipStreamSynchronize(ln.stream);
            (void)hipStreamDestroy(ln.stream);
        }
        ln = Model::Lane();
    }
    m->next_lane = 0;
}

}  // namespace r3d
