// r3d_streams_link: one person across cameras - per scene the association of the cameras' tracks (the streams r3d_streams_assign
// keeps per camera) with a table of people by the distance of their world poses, the births and the ends of people, and the member
// table r3d_streams_fuse reads.  The routines the kernel (r3d_k_elementwise.hip) and the host hook
// (r3d_debug_streams_link_host) share, __host__ __device__ so that the hooks build runs the very same ones on the CPU: the state's
// words as the rule reads them, a stream's present joints, the cost of a person and a stream, step A's test of one link, step B's
// candidate test, pair key and birth, step C's member row, per-joint mean and per-person finish.  Integers decide first; the
// arithmetic is float64 with floating-point contraction OFF: every operation rounds once, joints and cameras are visited in
// ascending order and sums start from zero, the divisions and the square roots are the correctly rounded ones on both sides.  The
// reference is monocular and pre-associated and has no counterpart: include/ray3d_hip.h is the definition.  The ONE state word
// that becomes an index is a link word, and only through stream_link_word, its range check.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ray3d_hip.h"
#include "r3d_streams_assign.hpp"      // STREAM_ASSIGN_NONE, stream_assign_better, stream_assign_greedy, stream_assign_nth_bit
#include "r3d_streams_fuse.hpp"        // stream_fuse_q, stream_finite_bits64, stream_finished

// On the device: the instruction scheduler does not move anything across this point - one float64 division's temporaries at a time
// instead of three interleaved ones, which is what keeps the kernel's other modes at their register count.  Nothing on the host.
#if defined(__HIP_DEVICE_COMPILE__)
#define STREAM_LINK_ONE_AT_A_TIME() __builtin_amdgcn_sched_barrier(0)
#else
#define STREAM_LINK_ONE_AT_A_TIME() ((void)0)
#endif

namespace r3d {

// r3d_streams_link: the arguments of r3d_k_streams_link.  blockIdx.x names a
// scene; the workgroup is one wavefront.
struct StreamsLinkArgs {
    void *state;                        // next_id[N], pid[NG], link_id[NG][C], ref[NG][J][3], phase, missed, link[NG][C], seen
    const double *world;                // (S, J, 3): what r3d_streams_poses wrote
    const long long *emit;              // S words of r3d_streams_step
    const int32_t *status;              // S words of r3d_streams_step
    const long long *id;                // (S) track identities, < 0: no track
    int32_t *member;                    // (N * G, M)
    long long *person;                  // (N * G)
    int32_t *group;                     // (S) or nullptr
    int32_t *stats;                     // (N, 4) or nullptr
    double max_dist, break_dist;        // > 0; <= 0: off
    int N, C, P, G, M, J, min_joints, min_common, max_missed;
};

constexpr int STREAMS_LINK_THREADS = 64;      // one wavefront per scene: its lanes own people, slots, then pairs
// The kernel's LDS: the G x P cost keys (at most 32 x 32 of 8 bytes), then the slots' present masks
constexpr int STREAMS_LINK_LDS_KEYS = 0;
constexpr int STREAMS_LINK_LDS_PRES = 8 * R3D_LINK_MAX_PEOPLE * R3D_ASSIGN_MAX_SLOTS;
constexpr int STREAMS_LINK_LDS_BYTES = STREAMS_LINK_LDS_PRES + 4 * R3D_ASSIGN_MAX_SLOTS;
static_assert(R3D_LINK_MAX_PEOPLE <= 32 && R3D_ASSIGN_MAX_SLOTS <= 32, "people and slots are bits of 32-bit masks");
static_assert(R3D_LINK_MAX_PEOPLE <= STREAMS_LINK_THREADS && R3D_ASSIGN_MAX_SLOTS <= STREAMS_LINK_THREADS, "one lane per person, one lane per slot");
static_assert(STREAMS_LINK_THREADS == STREAMS_ASSIGN_THREADS, "stream_assign_greedy's butterfly spans the wavefront of either kernel");

// bytes of the state (the arguments passed the shape rules: no overflow), rounded up to 8
inline size_t streams_link_bytes(long long N, long long C, long long G, long long J) {
    const long long NG = N * G;
    const long long bytes = 8 * N + NG * (8 + 8 * C + 24 * J + 4 + 4 + 4 * C + 4);
    return (size_t)((bytes + 7) / 8 * 8);
}

// The state's arrays, in the header's order
struct StreamLinkState {
    long long *next_id;                 // [N]
    long long *pid;                     // [NG]
    long long *link_id;                 // [NG][C]
    double *ref;                        // [NG][J][3]
    int32_t *phase, *missed;            // [NG] each
    int32_t *link;                      // [NG][C]: slot plus one
    uint32_t *seen;                     // [NG]
};
__host__ __device__ inline StreamLinkState stream_link_state(const StreamsLinkArgs &a) {
    const long long NG = (long long)a.N * a.G;
    StreamLinkState st;
    st.next_id = static_cast<long long *>(a.state);
    st.pid = st.next_id + a.N;
    st.link_id = st.pid + NG;
    st.ref = reinterpret_cast<double *>(st.link_id + NG * a.C);
    st.phase = reinterpret_cast<int32_t *>(st.ref + NG * a.J * 3);
    st.missed = st.phase + NG;
    st.link = st.missed + NG;
    st.seen = reinterpret_cast<uint32_t *>(st.link + NG * a.C);
    return st;
}

// A link word as the rule reads it: slot plus one in 1..P, anything else 0 (none).  THE range check: what it returns, minus one, is
// the only index the call ever takes from the state.
__host__ __device__ inline int stream_link_word(int32_t word, int P) { return word >= 1 && word <= P ? word : 0; }

// The bits of `seen` the rule reads
__host__ __device__ inline uint32_t stream_link_seen(uint32_t word, int J) { return word & (0xffffffffu >> (32 - J)); }     // (1 <= J <= 17)

// The absolute stream index of slot p of camera c of scene n
// (S and N * G are at most R3D_CLIPS_MAX, so streams, people and every element index below fit 32 unsigned bits: the device then
// addresses with a scalar base and a 32-bit lane offset)
__host__ __device__ inline uint32_t stream_link_stream(const StreamsLinkArgs &a, int n, int c, int p) { return (uint32_t)((n * a.C + c) * a.P + p); }

// The joints of stream s whose three world components are finite (the exponent bits)
__host__ __device__ inline uint32_t stream_link_present(const StreamsLinkArgs &a, uint32_t s) {
    uint32_t m = 0;
    const double *w = a.world + 3 * (s * a.J);
#pragma unroll 1
    for (int j = 0; j < a.J; ++j) {                     // (no branch: a joint's three loads are in flight together)
        const uint32_t ok = (uint32_t)stream_finite_bits64(w[3 * j]) & (uint32_t)stream_finite_bits64(w[3 * j + 1]) & (uint32_t)stream_finite_bits64(w[3 * j + 2]);
        m |= ok << j;
    }
    return m;
}

// cost(gi, s) over the joints of `common` (not empty): (sum of the distances) / their number.  Every joint's distance is formed -
// j < J lies inside both rows, whatever they hold - and only the common ones are summed: no branch around the loads.
__host__ __device__ inline double stream_link_cost(const StreamsLinkArgs &a, const StreamLinkState &st, uint32_t gi, uint32_t s, uint32_t common) {
#pragma clang fp contract(off)
    const double *world = a.world, *ref = st.ref;       // (scalar bases; the lane's part of an address is one 32-bit offset)
    uint32_t w = 3u * (s * (uint32_t)a.J), r = 3u * (gi * (uint32_t)a.J);
    double sum = 0.0;
#pragma unroll 1
    for (int j = 0; j < a.J; ++j, w += 3u, r += 3u) {
        const double q = stream_fuse_q(world[w], world[w + 1u], world[w + 2u], ref[r], ref[r + 1u], ref[r + 2u]);
        const double dist = sqrt(q);
        const double with = sum + dist;
        sum = ((common >> j) & 1u) ? with : sum;
    }
    return sum / (double)__builtin_popcount(common);
}

// Step A without its duplicate rule: the link of live person gi (absolute) in camera c of scene n as it stands after the identity
// and the break tests - slot plus one, or 0
__host__ __device__ inline int stream_link_validate(const StreamsLinkArgs &a, const StreamLinkState &st, int n, uint32_t gi, int c) {
    const int p1 = stream_link_word(st.link[gi * a.C + c], a.P);
    if (p1 == 0) return 0;
    const uint32_t s = stream_link_stream(a, n, c, p1 - 1);          // (p1 - 1 < P: the range check above)
    const long long id = a.id[s];
    if (id < 0 || id != st.link_id[gi * a.C + c]) return 0;           // the track ended or the slot was reused
    if (a.break_dist > 0.0 && stream_finished(a.status[s], a.emit[s])) {
        const uint32_t common = stream_link_present(a, s) & stream_link_seen(st.seen[gi], a.J);
        if (common && stream_link_cost(a, st, gi, s, common) > a.break_dist) return 0;      // (a NaN cost keeps the link)
    }
    return p1;
}

// Step B: slot p of camera c is a candidate - a track that finished this tick, held by nobody (`held`: the camera's slots some
// person holds), with min_joints present joints; *present is the stream's mask when it finished, else 0
__host__ __device__ inline bool stream_link_candidate(const StreamsLinkArgs &a, int n, int c, int p, uint32_t held, uint32_t *present) {
    const uint32_t s = stream_link_stream(a, n, c, p);
    *present = 0;
    if (!stream_finished(a.status[s], a.emit[s])) return false;
    *present = stream_link_present(a, s);
    return a.id[s] >= 0 && !((held >> p) & 1u) && __builtin_popcount(*present) >= a.min_joints;
}

// Step B: the cost key of eligible person g and candidate slot p of camera c - the bits of the cost, or STREAM_ASSIGN_NONE when the
// common joints are too few or the cost is not <= max_dist (a NaN fails)
__host__ __device__ inline unsigned long long stream_link_pair(const StreamsLinkArgs &a, const StreamLinkState &st, int n, int g, int c, int p,
                                                               uint32_t present) {
    const uint32_t gi = (uint32_t)(n * a.G + g);
    const uint32_t common = present & stream_link_seen(st.seen[gi], a.J);
    const int k = __builtin_popcount(common);
    if (k < 1 || k < a.min_common) return STREAM_ASSIGN_NONE;
    const double cost = stream_link_cost(a, st, gi, stream_link_stream(a, n, c, p), common);
    if (!(cost <= a.max_dist)) return STREAM_ASSIGN_NONE;
    return __builtin_bit_cast(unsigned long long, cost);
}

// Step B: person gi is born from stream s with identity pid: its words but the links, which the caller writes
__host__ __device__ inline void stream_link_birth(const StreamsLinkArgs &a, const StreamLinkState &st, uint32_t gi, uint32_t s, long long pid) {
    const uint32_t present = stream_link_present(a, s);
    const double *w = a.world + 3 * (s * a.J);
    double *ref = st.ref + 3 * (gi * a.J);
#pragma unroll 1
    for (int j = 0; j < a.J; ++j)
        if ((present >> j) & 1u) {
            ref[3 * j] = w[3 * j];
            ref[3 * j + 1] = w[3 * j + 1];
            ref[3 * j + 2] = w[3 * j + 2];
        }
    st.pid[gi] = pid;
    st.phase[gi] = 1;
    st.missed[gi] = 0;
    st.seen[gi] = present;
}

// Camera c's link of person gi as the call leaves it: the state's word (every link word is written on every call, 0 for a person
// that is not live), the identity of a link made in this call, and the member table's slot
__host__ __device__ inline void stream_link_store(const StreamsLinkArgs &a, const StreamLinkState &st, int n, uint32_t gi, int c, int p1, bool made) {
    st.link[gi * a.C + c] = p1;
    const uint32_t s = stream_link_stream(a, n, c, p1 ? p1 - 1 : 0);
    if (made) st.link_id[gi * a.C + c] = a.id[s];        // (made: p1 != 0)
    a.member[gi * a.M + c] = p1 ? (int32_t)s : -1;        // (s < S <= R3D_CLIPS_MAX)
}

// Step C, first the members: after every camera's stream_link_store, the row of live person gi - tbl[c] = the stream of its link
// in camera c when that stream finished this tick, else -1 -> the person has a link at all
__host__ __device__ inline bool stream_link_members(const StreamsLinkArgs &a, const StreamLinkState &st, int n, uint32_t gi, int32_t *tbl) {
    bool linked = false;
    for (int c = 0; c < a.C; ++c) {
        const int p1 = stream_link_word(st.link[gi * a.C + c], a.P);
        int32_t s = -1;
        if (p1) {
            linked = true;
            const uint32_t at = stream_link_stream(a, n, c, p1 - 1);
            if (stream_finished(a.status[at], a.emit[at])) s = (int32_t)at;
        }
        tbl[c] = s;
    }
    return linked;
}

// Step C, then joint j of live person gi: over the members of `tbl` that have the joint present, cameras in ascending order, ref[j]
// becomes the mean of their points -> there was such a member
__host__ __device__ inline bool stream_link_joint(const StreamsLinkArgs &a, const StreamLinkState &st, uint32_t gi, int j, const int32_t *tbl) {
#pragma clang fp contract(off)
    double x = 0.0, y = 0.0, z = 0.0;
    int k = 0;
    for (int c = 0; c < a.C; ++c) {
        const int32_t s = tbl[c];
        if (s < 0) continue;
        const double *w = a.world + 3 * ((uint32_t)s * a.J + j);
        const double wx = w[0], wy = w[1], wz = w[2];
        if (!(stream_finite_bits64(wx) && stream_finite_bits64(wy) && stream_finite_bits64(wz))) continue;
        x = x + wx;
        y = y + wy;
        z = z + wz;
        ++k;
    }
    if (k == 0) return false;
    const double kk = (double)k;
    double *ref = st.ref + 3 * (gi * a.J + j);
    ref[0] = x / kk;
    STREAM_LINK_ONE_AT_A_TIME();
    ref[1] = y / kk;
    STREAM_LINK_ONE_AT_A_TIME();
    ref[2] = z / kk;
    return true;
}

// Step C, last the person gi itself; `alive`: live at entry or born in this call; `linked`: stream_link_members; `add`: the joints
// stream_link_joint gave a point.  Also the person's row of person_dev and the member table's slots C .. M - 1 -> live after the call.
__host__ __device__ inline bool stream_link_person(const StreamsLinkArgs &a, const StreamLinkState &st, uint32_t gi, bool alive, bool linked, uint32_t add) {
    for (int m = a.C; m < a.M; ++m) a.member[gi * a.M + m] = -1;
    if (!alive) {
        a.person[gi] = -1;
        return false;
    }
    if (add) st.seen[gi] |= add;                        // (the word's bits J .. 31 stay as they are)
    bool live = true;
    if (linked) {
        st.missed[gi] = 0;
    } else {
        int missed = st.missed[gi];
        if (missed < 0) missed = 0;
        if (missed >= a.max_missed) {                   // (missed + 1 > max_missed, without the overflow): the person is freed
            st.phase[gi] = 0;
            live = false;
        } else {
            st.missed[gi] = missed + 1;
        }
    }
    a.person[gi] = live ? st.pid[gi] : -1;
    return live;
}

}  // namespace r3d
