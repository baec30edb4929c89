// The elementwise kernels: the pixel pre-pass of the forwards and one kernel per elementwise entry point of include/ray3d_hip.h
// (r3d_clips_*, r3d_finalize_dev's pack, r3d_streams_*).  One translation unit and so one code object, loaded at once.  Each kernel
// takes its own argument struct by value and runs one workgroup body below; the per-point arithmetic lives in the r3d_*.hpp headers,
// __host__ __device__, where the hooks build's host copies run the very same routines.  Plain vector stores from C++ throughout;
// the one atomic is r3d_clips_project's integer count of points outside the frame.
#include "r3d_internal.hpp"
#include "r3d_clips_repair.hpp"
#include "r3d_pack.hpp"
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
#include "r3d_windows.hpp"

namespace r3d {

__device__ __forceinline__ void undistort_body(const UndistArgs &a) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.npts) return;
    int src = p, w;
    if (a.pts_per_window > 0) {              // materialised (B, RF, J, F): window w's RF frames, read from the sliding input
        w = p / a.pts_per_window;
        src = w * a.window_stride * a.J + (p - w * a.pts_per_window);
    } else {                                 // one point per input frame: frame f belongs to window min(f / stride, B - 1)
        w = min(p / a.J / a.window_stride, a.last_window);
    }
    const double *row = a.cam + (long long)w * a.cam_stride;
    const double u = (double)a.uv[2 * (long long)src], v = (double)a.uv[2 * (long long)src + 1];
    const int F = enc_floats(a.encoding);
    const EncodedPoint e = encode_point_f32(row, a.encoding, u, v);
    float *o = a.rays + F * (long long)p;
    o[0] = e.x;
    o[1] = e.y;
    if (F == 3) o[2] = e.z;
}

__device__ __forceinline__ void clips_encode_body(const ClipsEncArgs &c) {
    const r3d_clip_input_desc *d = c.table + blockIdx.y;
    const long long first = d->first_frame, n = d->n_frames, out_first = d->out_first;
    const int pad_front = d->pad_front, pad_back = d->pad_back;
    const bool ok = clip_input_valid(first, n, out_first, pad_front, pad_back, c.total_frames, c.out_rows, c.max_rows);
    if (blockIdx.x == 0 && threadIdx.x == 0) c.status[blockIdx.y] = ok ? 0 : 1;
    if (!ok) return;                         // an invalid descriptor is not followed: nothing of the clip is read or written
    // (max_rows * J fits in 31 bits - checked on the host - and so do the clip's points and this launch's indices)
    const int npts = (int)(pad_front + n + pad_back) * c.J;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npts) return;                   // also the workgroups past the clip's own count
    const int r = p / c.J, j = p - r * c.J;
    const long long src = (first + clip_input_source(r, pad_front, n)) * c.J + j;
    const long long row0 = (out_first + r) * c.J;
    const int F = enc_floats(c.encoding);
    const EncodedPoint e = encode_point_f32(d->cam, c.encoding, (double)c.px[2 * src], (double)c.px[2 * src + 1]);
    float *o = c.x + F * (row0 + j);
    o[0] = e.x;
    o[1] = e.y;
    if (F == 3) o[2] = e.z;
    if (c.x_mirror) {                        // trainer.py:299-302 on the encoded input: x -> -x (exact), left <-> right
        float *m = c.x_mirror + F * (row0 + mirror_dest(c.mirror_inv[0], c.mirror_inv[1], j));
        m[0] = -e.x;
        m[1] = e.y;
        if (F == 3) m[2] = e.z;
    }
}

__device__ __forceinline__ void clips_poses_body(const ClipsPosesArgs &q) {
    const r3d_clip_desc *d = q.table + blockIdx.y;
    const long long first = d->first_frame, n = d->n_frames, raw_first = q.raw_first[blockIdx.y];
    const bool ok = clip_pose_valid(first, n, raw_first, q.total_frames, q.max_frames, q.raw_rows);
    if (blockIdx.x == 0 && threadIdx.x == 0) q.status[blockIdx.y] = ok ? 0 : 1;
    if (!ok) return;                         // an invalid descriptor is not followed: nothing of the clip is read or written
    // (max_frames * J fits in 31 bits - checked on the host - and so do the clip's points and this launch's indices)
    const int npts = (int)n * q.J;
    const int pt = blockIdx.x * blockDim.x + threadIdx.x;
    if (pt >= npts) return;                  // also the workgroups past the clip's own count
    const int f = pt / q.J, j = pt - f * q.J;
    const long long src_row = (raw_first + f) * q.J;
    const float *mir = q.raw_mirror ? q.raw_mirror + 3 * (src_row + pose_mirror_source(q.mirror_perm[0], q.mirror_perm[1], j)) : nullptr;
    float p[3];
    pose_finish(q.raw + 3 * (src_row + j), mir, p);
    const long long dst = 3 * ((first + f) * q.J + j);
    if (q.pred) {
        q.pred[dst] = p[0];
        q.pred[dst + 1] = p[1];
        q.pred[dst + 2] = p[2];
    }
    if (q.world) {
        double w[3];
        pose_world(d->rn2w, d->tn2w, p, w);
        q.world[dst] = w[0];
        q.world[dst + 1] = w[1];
        q.world[dst + 2] = w[2];
    }
}

__device__ __forceinline__ void clips_project_body(const ClipsProjectArgs &g) {
    const r3d_clip_project_desc *d = g.table + blockIdx.y;
    const long long first = d->first_frame, n = d->n_frames, out_first = d->out_first, gt_first = d->gt_first;
    const int pad_front = d->pad_front, pad_back = d->pad_back;
    const bool ok = clip_project_valid(first, n, out_first, pad_front, pad_back, gt_first, g.total_frames, g.out_rows, g.max_rows, g.gt_rows,
                                       g.gt != nullptr || g.px != nullptr);
    if (blockIdx.x == 0 && threadIdx.x == 0) g.status[blockIdx.y] = ok ? 0 : 1;
    if (!ok) return;                         // an invalid descriptor is not followed: nothing of it is read or written
    // (max_rows * J fits in 31 bits - checked on the host - and so do the clip's points and this launch's indices)
    const int npts = (int)(pad_front + n + pad_back) * g.J;
    if ((int)(blockIdx.x * blockDim.x) >= npts) return;      // uniform: the workgroups past the clip's own count
    const int pt = blockIdx.x * blockDim.x + threadIdx.x;
    bool outside = false;                    // (no thread leaves before the wavefront's count below)
    if (pt < npts) {
        const int r = pt / g.J, j = pt - r * g.J;
        const float *src = g.world + 3 * ((first + clip_input_source(r, pad_front, n)) * g.J + j);
        const float p[3] = {src[0], src[1], src[2]};
        double u, v;
        project_pixel(d->proj, p, u, v);
        const long long row0 = (out_first + r) * g.J;
        const int F = enc_floats(g.encoding);
        const EncodedPoint e = encode_point_f32(d->cam, g.encoding, u, v);
        float *o = g.x + F * (row0 + j);
        o[0] = e.x;
        o[1] = e.y;
        if (F == 3) o[2] = e.z;
        if (g.x_mirror) {                    // r3d_clips_encode's rule: x -> -x (exact), left <-> right
            float *m = g.x_mirror + F * (row0 + mirror_dest(g.mirror_inv[0], g.mirror_inv[1], j));
            m[0] = -e.x;
            m[1] = e.y;
            if (F == 3) m[2] = e.z;
        }
        const long long f = (long long)r - pad_front;
        if (f >= 0 && f < n) {               // the unpadded rows: every source frame once
            const long long at = (gt_first + f) * g.J + j;
            if (g.gt) {
                double w[3];
                pose_world(d->rw2g, d->tw2g, p, w);
                g.gt[3 * at] = encoded_f32(w[0]);
                g.gt[3 * at + 1] = encoded_f32(w[1]);
                g.gt[3 * at + 2] = encoded_f32(w[2]);
            }
            if (g.px) {
                g.px[2 * at] = pose_f64(u);
                g.px[2 * at + 1] = pose_f64(v);
            }
            outside = pixel_outside(u, v, d->cam[UNDIST_ROW_RES_W], d->cam[UNDIST_ROW_RES_H]);
        }
    }
    if (g.outside) {                         // uniform.  One integer add per wavefront that saw a point outside the frame
        const unsigned long long seen = __ballot(outside);
        if (seen && (threadIdx.x & (warpSize - 1)) == 0) atomicAdd(g.outside + blockIdx.y, (int)__popcll(seen));
    }
}

__device__ __forceinline__ void pack_body(const PackArgs &k) {
    int lo = 0, hi = k.nseg - 1;             // the last segment that starts at or before this workgroup (the list is sorted, blk0[0] == 0)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (k.segs[mid].blk0 <= (int)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const PackSeg sg = k.segs[lo];
    const int blk = (int)blockIdx.x - sg.blk0;
    if (blk >= sg.nblk) return;              // (the grid is exactly the segments' workgroups: never taken)
    pack_item(k, sg, blk * PACK_THREADS + (int)threadIdx.x);
}

__device__ __forceinline__ void clips_windows_body(const WindowsArgs &v) {
    const WindowRun q = window_lookup(v, blockIdx.y);          // uniform: blockIdx.y < batch, the run index inside [0, num_runs)
    if (blockIdx.x == 0 && threadIdx.x == 0 && (!q.ok || q.member)) v.status[q.r] = q.ok ? 0 : 1;
    if (!q.member) return;                   // an invalid descriptor is not followed; a window no run holds is left untouched
    if (v.param && blockIdx.x == 0)          // uniform.  The run's parameter row beside the window
        for (int e = threadIdx.x; e < v.E; e += blockDim.x) v.param[(long long)blockIdx.y * v.E + e] = v.run_param[(long long)q.r * v.E + e];
    // (RF * J and batch * RF * J fit in 31 bits - checked on the host)
    const int pt = blockIdx.x * blockDim.x + threadIdx.x;
    if (pt >= v.RF * v.J) return;
    const int i = pt / v.J, j = pt - i * v.J;
    uint32_t o[3];
    window_point(v, q.first + window_source_frame(q.start, q.k, q.step, i, q.n), q.flip, j, o);
    uint32_t *dst = v.x + v.F * ((long long)blockIdx.y * (v.RF * v.J) + pt);
    dst[0] = o[0];
    dst[1] = o[1];
    if (v.F == 3) dst[2] = o[2];
}

// The advance launch: stream blockIdx.x < S.  The head and the action word are the same for every thread of the workgroup, so the
// verdict is uniform; the workgroup is ONE wavefront (launch_streams_step), and the barrier in front of the head's store keeps the
// order also for a wider one: every load of the head is done before thread 0 replaces it.
__device__ __forceinline__ void streams_advance_body(const StreamsArgs &t) {
    const int s = blockIdx.x;
    const long long count = t.heads[s].count, drained = t.heads[s].drained;
    const StreamStep st = stream_step(count, drained, t.action[s], t.lag, t.RF);
    if (st.push && (int)threadIdx.x < t.J) stream_store_point(t, s, st.slot, threadIdx.x);     // (slot < RF, j < J: inside ring s)
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (st.write_head) {
        t.heads[s].count = st.count;
        t.heads[s].drained = st.drained;
    }
    t.emit[s] = st.emit;
    t.status[s] = st.refused ? 1 : 0;
}

// The gather launch: stream blockIdx.y < S, output point blockIdx.x * 256 + threadIdx.x of its window
__device__ __forceinline__ void streams_gather_body(const StreamsArgs &t) {
    const int s = blockIdx.y;
    const long long c = t.heads[s].count, n = t.emit[s];
    if (!stream_emits(c, t.heads[s].drained, n, t.status[s], t.lag)) return;      // uniform: the stream's row is left untouched
    // (RF * J and S * RF * J fit in 31 bits - checked on the host)
    const int pt = blockIdx.x * blockDim.x + threadIdx.x;
    if (pt >= t.RF * t.J) return;
    const int i = pt / t.J;
    stream_gather_point(t, s, n, c, i, pt - i * t.J);
}

// Stream blockIdx.x < S, joint threadIdx.x < J <= 17.  emit[s] and status[s] are one address for the workgroup, so the verdict is
// uniform and an unfinished stream's workgroup leaves before the barrier as a whole: nothing of its rows is read or written.
__device__ __forceinline__ void streams_poses_body(const StreamsPosesArgs &u) {
    __shared__ double res[17];
    const int s = blockIdx.x;
    if (!stream_finished(u.status[s], u.emit[s])) return;
    const int j = threadIdx.x;
    if (j < u.J) {
        const double e = stream_pose_point(u, s, j);                 // (s < S, j < J: inside rows s of every buffer)
        if (u.quality) res[j] = e;
    }
    if (!u.quality) return;                  // uniform
    __syncthreads();
    if (j != 0) return;
    double qw[2];
    stream_quality(res, u.J, qw);
    u.quality[2 * s] = qw[0];
    u.quality[2 * s + 1] = qw[1];
}

// Stream blockIdx.x < S, joint threadIdx.x < J <= 17; the workgroup is ONE wavefront (launch_streams_repair).  The head and the action
// word are one address for the workgroup, so the verdict is uniform and both barriers are reached by every thread or by none.
__device__ __forceinline__ void streams_repair_body(const StreamsRepairArgs &r) {
    const int s = blockIdx.x, j = threadIdx.x;
    const StreamRepairStep rs = stream_repair_step(r, s);
    if (!rs.st.push) {                       // uniform: IDLE, DRAIN, a refused stream - nothing of its track, ring or row is written
        if (j == 0) r.synthetic[s] = stream_repair_idle_word(r, s, rs.st);
        return;
    }
    if (rs.restart) {                        // uniform: the track is zeroed first (every word by one thread), whatever it held
        for (int i = j; i < stream_repair_track_words(r); i += blockDim.x) stream_repair_zero(r, s, i);
        __syncthreads();
    }
    bool miss = false;
    if (j < r.J) miss = stream_repair_joint(r, s, j, rs.c, rs.restart);        // (s < S, j < J: inside rows s of every buffer)
    const unsigned long long mask = __ballot(miss);                             // (no thread left before it; bit j: thread j < J <= 17)
    if (j == 0) stream_repair_finish(r, s, rs.c, (uint32_t)mask);
}

// Stream blockIdx.y < S, look blockIdx.z < K, output point blockIdx.x * 256 + threadIdx.x of the preview window.  The head, the action
// and the status word are one address for the workgroup, so the verdict is uniform and comes before any store; the state is only
// read, and what the launch writes - row block (k, s) and its two words - no other workgroup of it reads.
__device__ __forceinline__ void streams_peek_body(const StreamsPeekArgs &e) {
    const int s = blockIdx.y, k = blockIdx.z;
    const long long c = e.heads[s].count;
    const StreamPeek pk = stream_peek(c, e.heads[s].drained, e.action != nullptr, e.action ? e.action[s] : R3D_STREAM_PUSH, e.status[s],
                                      stream_peek_look(e, k), e.lag);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        e.emit[(long long)k * e.S + s] = pk.p;          // (-1 unless the stream previews)
        e.peek_status[(long long)k * e.S + s] = pk.bad ? 1 : 0;
    }
    if (!pk.previews) return;                // uniform: the row block is left untouched
    // (RF * J and K * S * RF * J fit in 31 bits - checked on the host)
    const int pt = blockIdx.x * blockDim.x + threadIdx.x;
    if (pt >= e.RF * e.J) return;
    const int i = pt / e.J;
    stream_peek_point(e, k, s, pk.p, c, i, pt - i * e.J);
}

// Group blockIdx.x < G, joint threadIdx.x < J <= 17; the workgroup is ONE wavefront (launch_streams_fuse).  No thread leaves before the
// ballots; `used` and M are the same for every thread, so the loop around them is uniform.
__device__ __forceinline__ void streams_fuse_body(const StreamsFuseArgs &f, double *stage) {
    const int g = blockIdx.x, j = threadIdx.x;
    uint32_t inl = 0;
    if (j < f.J) inl = stream_fuse_joint(f, g, j, stage + j, STREAMS_FUSE_JOINTS);     // (g < G, j < J <= 17: column j of the staging area)
    if (!f.used) return;                     // uniform
    for (int m = 0; m < f.M; ++m) {
        const unsigned long long mask = __ballot((inl >> m) & 1u);                     // (bit j: thread j < J <= 17)
        if (j == 0) f.used[(long long)g * f.M + m] = (uint32_t)mask;
    }
}

// Camera blockIdx.x < C; the workgroup is ONE wavefront (launch_streams_assign) and no lane leaves before the last ballot: every
// loop bound and every branch around a barrier, a shuffle or a ballot is the same for all 64 lanes.  `lds`: STREAMS_ASSIGN_LDS_BYTES.
__device__ __forceinline__ void streams_assign_body(const StreamsAssignArgs &a, unsigned char *lds) {
    unsigned long long *key = reinterpret_cast<unsigned long long *>(lds + STREAMS_ASSIGN_LDS_KEYS);       // [p * D + d], p < P, d < D
    double *size = reinterpret_cast<double *>(lds + STREAMS_ASSIGN_LDS_SIZE);                              // [d], d < D <= 32
    uint32_t *obs = reinterpret_cast<uint32_t *>(lds + STREAMS_ASSIGN_LDS_OBS);                            // [d], d < D <= 32
    const int c = blockIdx.x, lane = threadIdx.x;
    const StreamAssignState st = stream_assign_state(a);
    const int n = stream_assign_count(a.det_count[c], a.D);         // (one address for the workgroup; the clamp: n <= D)
    // step 1: lane d < n <= D owns detection d
    StreamAssignDet det = {0u, 0.0, false};
    if (lane < n) det = stream_assign_detection(a, c, lane);
    if (lane < a.D) {
        size[lane] = det.size;
        obs[lane] = det.obs;
    }
    const uint32_t valid = (uint32_t)__ballot(det.valid);           // (bit d: lane d < n <= 32)
    __syncthreads();
    // step 2: lane (d, half) = (lane % 32, lane / 32) owns the pairs (p, d) with p = half, half + 2, ... < P of its column d < D:
    // no division, one reference row per half wavefront and step
    const int d = lane & 31, half = lane >> 5;
    if (d < a.D) {
        const StreamAssignDet dd = {obs[d], size[d], ((valid >> d) & 1u) != 0};
        for (int p = half; p < a.P; p += 2) key[p * a.D + d] = stream_assign_pair(a, st, c, p, d, dd);      // (p < P, d < D)
    }
    __syncthreads();
    // step 3: the greedy matching; `rows`, `cols` and the winner are the same in every lane
    uint32_t rows = 0, cols = 0;
    int matched = -1;
    stream_assign_greedy(key, a.P, a.D, rows, cols, [&](int wp, int wd) {
        if (lane == wp) matched = wd;
    });
    // steps 4 to 7: lane p < P owns slot p
    const int phase = lane < a.P ? stream_assign_phase(st.phase[(long long)c * a.P + lane], a.lag) : -1;
    const uint32_t free_mask = (uint32_t)__ballot(phase == 0);      // (bit p: lane p < P <= 32)
    const uint32_t unmatched = valid & ~cols;
    const long long next = st.next_id[c];                           // (every lane reads it before lane 0 replaces it below)
    if (lane < a.P) stream_assign_slot(a, st, c, lane, matched, free_mask, unmatched, next);
    if (lane == 0) stream_assign_finish(a, st, c, valid, cols, free_mask, unmatched, next);
}

// Scene blockIdx.x < N; the workgroup is ONE wavefront (launch_streams_link) and no lane leaves before the last ballot: the camera
// loop, every other loop bound and every branch around a barrier, a shuffle or a ballot is the same for all 64 lanes.  Lanes G .. 63
// own no person and lanes P .. 63 no slot: they take part in the ballots with `false`.  `lds`: STREAMS_LINK_LDS_BYTES.
__device__ __forceinline__ void streams_link_body(const StreamsLinkArgs &a, unsigned char *lds) {
    unsigned long long *key = reinterpret_cast<unsigned long long *>(lds + STREAMS_LINK_LDS_KEYS);         // [g * P + p], g < G, p < P
    uint32_t *pres = reinterpret_cast<uint32_t *>(lds + STREAMS_LINK_LDS_PRES);                            // [p], p < P <= 32
    const int n = blockIdx.x, lane = threadIdx.x;
    const StreamLinkState st = stream_link_state(a);
    const bool mine = lane < a.G;                                   // lane g < G owns person g
    const uint32_t gi = (uint32_t)(n * a.G + (mine ? lane : 0));    // (gi < N * G <= R3D_CLIPS_MAX in every lane)
    const uint32_t below = (1u << (lane & 31)) - 1u;                // the people / slots in front of this lane's
    const bool entry = mine && st.phase[gi] == 1;                   // live at entry
    bool alive = entry;                                             // ... or born in this call
    long long next = st.next_id[n];                                 // (lane 0 replaces it after the last camera)
    int links = 0, births = 0, dropped = 0;
    const int pl = lane & 31, half = lane >> 5;
    for (int c = 0; c < a.C; ++c) {
        // step A: lane g tests its link; of several people on one stream the smallest g keeps it
        int p1 = entry ? stream_link_validate(a, st, n, gi, c) : 0;
        uint32_t held = 0;
        for (int p = 0; p < a.P; ++p) {
            const uint32_t m = (uint32_t)__ballot(p1 == p + 1);     // (bit g: lane g < G <= 32)
            if (m) held |= 1u << p;
            if (p1 == p + 1 && (m & below)) p1 = 0;
        }
        // step B: lane p < P summarises slot p
        uint32_t present = 0;
        const bool candidate = lane < a.P && stream_link_candidate(a, n, c, lane, held, &present);
        if (lane < a.P) pres[lane] = present;
        const uint32_t cand = (uint32_t)__ballot(candidate);        // (bit p: lane p < P <= 32)
        // (a person's seen word in memory is current: nobody writes it before step C but its own birth, by this lane)
        const uint32_t elig = (uint32_t)__ballot(alive && p1 == 0 && stream_link_seen(st.seen[gi], a.J) != 0u);
        uint32_t rows = 0, cols = 0;
        bool made = false;
        if (cand && elig) {                                         // uniform
            __syncthreads();
            // lane (p, half) = (lane % 32, lane / 32) owns the pairs (g, p) with g = half, half + 2, ... < G of its column p < P
            if (pl < a.P)
                for (int g = half; g < a.G; g += 2)
                    key[g * a.P + pl] = ((cand >> pl) & (elig >> g) & 1u) ? stream_link_pair(a, st, n, g, c, pl, pres[pl]) : STREAM_ASSIGN_NONE;
            __syncthreads();
            // the greedy matching; `rows`, `cols` and the winner are the same in every lane
            stream_assign_greedy(key, a.G, a.P, rows, cols, [&](int wg, int wp) {
                if (lane == wg) {
                    p1 = wp + 1;
                    made = true;
                }
            });
        }
        // births: the rank-th unmatched candidate takes the rank-th free person
        const uint32_t unmatched = cand & ~cols;
        const uint32_t free_mask = (uint32_t)__ballot(mine && !alive);
        const int want = __builtin_popcount(unmatched), room = __builtin_popcount(free_mask);
        const int born = want < room ? want : room;
        if (mine && !alive) {
            const int rank = __builtin_popcount(free_mask & below);
            if (rank < want) {
                const int p = stream_assign_nth_bit(unmatched, rank);      // (a bit of cand: p < P)
                stream_link_birth(a, st, gi, stream_link_stream(a, n, c, p), (long long)((unsigned long long)next + (unsigned long long)rank));
                alive = true;
                p1 = p + 1;
                made = true;
            }
        }
        next = (long long)((unsigned long long)next + (unsigned long long)born);
        links += __builtin_popcount(cols);
        births += born;
        dropped += want - born;
        if (mine) stream_link_store(a, st, n, gi, c, p1, made);
        if (a.group)                                                // uniform
            for (int p = 0; p < a.P; ++p) {
                const uint32_t m = (uint32_t)__ballot(p1 == p + 1);     // (at most one bit)
                if (lane == p) a.group[stream_link_stream(a, n, c, p)] = m ? n * a.G + __builtin_ctz(m) : -1;
            }
        __syncthreads();        // a born person's words are in memory before camera c + 1's keys are formed; the LDS is free again
    }
    // step C: lane g lists person g's finished members in LDS (the keys' block is free now); then lane (j, half) forms joint j of the
    // people of its parity - consecutive lanes read consecutive points -, the ballot of "got a point" is the person's new seen bits;
    // then lane g finishes person g
    int32_t *tbl = reinterpret_cast<int32_t *>(lds + STREAMS_LINK_LDS_KEYS);           // [g * C + c], g < G, c < C <= 16
    const bool linked = alive && stream_link_members(a, st, n, gi, tbl + lane * a.C);  // (alive: lane < G)
    const uint32_t alive_mask = (uint32_t)__ballot(alive);
    __syncthreads();
    for (int g0 = 0; g0 < a.G; g0 += 2) {                               // uniform: both halves make every turn
        const int g = g0 + half;
        const bool got = g < a.G && pl < a.J && ((alive_mask >> g) & 1u) && stream_link_joint(a, st, (uint32_t)(n * a.G + g), pl, tbl + g * a.C);
        const unsigned long long m = __ballot(got);
        if (pl == 0 && g < a.G) pres[g] = (uint32_t)(half ? m >> 32 : m);           // (bit j: lane j of the half; pres is free as well)
    }
    __syncthreads();
    const bool live = mine && stream_link_person(a, st, gi, alive, linked, pres[lane & 31]);
    const uint32_t lives = (uint32_t)__ballot(live);
    if (lane == 0) {
        st.next_id[n] = next;
        if (a.stats) {
            a.stats[4 * n] = __builtin_popcount(lives);
            a.stats[4 * n + 1] = links;
            a.stats[4 * n + 2] = births;
            a.stats[4 * n + 3] = dropped;
        }
    }
}

// Joint blockIdx.x < J of clip blockIdx.y: 256 threads, four wavefronts.  The descriptor is one address for the workgroup, so the
// verdict is uniform and a refused clip's workgroup leaves as a whole before any barrier; every loop bound is uniform, and no thread
// leaves before the last ballot or barrier: a thread past the clip's rows takes part with `false`.  `lds`: CLIPS_REPAIR_LDS_BYTES.
__device__ __forceinline__ void clips_repair_body(const ClipsRepairArgs &a, unsigned char *lds) {
    unsigned long long *bits = reinterpret_cast<unsigned long long *>(lds + CLIPS_REPAIR_LDS_BITS);   // [r / 64], r < R <= 65 536
    int32_t *wfirst = reinterpret_cast<int32_t *>(lds + CLIPS_REPAIR_LDS_FIRST);                      // [wave]
    int32_t *wcount = reinterpret_cast<int32_t *>(lds + CLIPS_REPAIR_LDS_COUNT);                      // [wave * 4 + counter]
    const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ClipRepairClip c = clip_repair_clip(a, a.table + blockIdx.y);
    if (j == 0 && tid == 0) a.status[blockIdx.y] = c.ok ? 0 : 1;
    if (!c.ok) return;                       // an invalid descriptor is not followed: nothing else of the clip is read or written
    // pass 1: the bitmap of observed rows; a step's four words are written whole, so rows R .. read as not observed
    int first = -1;                          // the first row this wavefront saw observed (the same in its 64 lanes)
    for (int base = 0; base < c.R; base += CLIPS_REPAIR_THREADS) {
        const int r = base + tid;
        const unsigned long long m = __ballot(r < c.R && clip_repair_observed(a, c, r, j));
        if (lane == 0) bits[(base >> 6) + wave] = m;            // (base + 255 < R + 255 <= 65 536 + 255, base a multiple of 256: word < 1 024)
        if (first < 0 && m) first = base + wave * 64 + __builtin_ctzll(m);
    }
    if (lane == 0) wfirst[wave] = first;
    __syncthreads();                         // the bitmap is whole, and every point was judged before any is rewritten
    first = -1;                              // min O
    for (int w = 0; w < CLIPS_REPAIR_WAVES; ++w) {
        const int f = wfirst[w];
        if (f >= 0 && (first < 0 || f < first)) first = f;
    }
    // pass 2: the missing points
    const int own0 = c.pad_front, own1 = c.pad_front + (int)c.n;    // the clip's own frames: what the counters count
    int carry = -1, cnt[4] = {0, 0, 0, 0};
    for (int base = 0; base < c.R; base += CLIPS_REPAIR_THREADS) {
        const int r = base + tid;
        int state = CLIP_REPAIR_OBSERVED;
        if (r < c.R) {
            if (!((bits[r >> 6] >> (r & 63)) & 1ull)) state = clip_repair_point(a, c, bits, first, clip_repair_prev(bits, r, carry), r, j);
            if (a.state) a.state[(c.out_first + r) * a.J + j] = (uint8_t)state;
        }
        if (a.stats) {                       // uniform
            const int mine = r >= own0 && r < own1 ? state : CLIP_REPAIR_OBSERVED;
            for (int k = 0; k < 4; ++k) cnt[k] += (int)__popcll(__ballot(mine == k + 1));
        }
        carry = clip_repair_carry(bits, base >> 6, carry);
    }
    if (!a.stats) return;                    // uniform
    if (lane == 0)
        for (int k = 0; k < 4; ++k) wcount[wave * 4 + k] = cnt[k];
    __syncthreads();
    if (tid != 0) return;
    int32_t *out = a.stats + ((long long)blockIdx.y * a.J + j) * 4;
    for (int k = 0; k < 4; ++k) out[k] = wcount[k] + wcount[4 + k] + wcount[8 + k] + wcount[12 + k];
}

// r3d_undistort_rays_f64: the pixel pre-pass of R3D_INPUT_UV_DIST, R3D_INPUT_PX_INTRINSIC and R3D_INPUT_PX_SCREEN
// (include/ray3d_hip.h).  Raw pixel keypoints in, the model's float32 input out - into the tail of the caller's workspace,
// where the R3D_INPUT_RAYS forward then reads it.  One keypoint per thread: its camera row (the row of the window the
// keypoint belongs to), the float64 routines of r3d_undistort.hpp, one cast to float32 as lib/train_val/trainer.py:298
// does.  `encoding` (uniform over the launch: scalar branches around the shared arithmetic) selects what is written:
//   ENC_RAY        five fixed-point iterations, re-projection, the 3-float ray (the kernel's name dates from this one);
//   ENC_INTRINSIC  the same undistortion, then the 2 floats ((u-cx)/fx, (v-cy)/fy) - the 2-feature models' input under
//                  INTRINSIC_ENCODING;
//   ENC_SCREEN     no undistortion: the 2 floats (u/w*2 - 1, v/w*2 - h/w) from the row's resolution slots.
// Memory-streaming elementwise work: consecutive threads read consecutive 8-byte pixel pairs and write consecutive 12-
// or 8-byte outputs; the camera rows (a few KiB for a batch) come from the caches.
extern "C" __global__ __launch_bounds__(256) void r3d_undistort_rays_f64(const UndistArgs a) { undistort_body(a); }

hipError_t launch_undistort(const UndistArgs &args, hipStream_t stream) {
    if (args.npts <= 0) return hipSuccess;
    r3d_undistort_rays_f64<<<dim3((args.npts + 255) / 256), dim3(256), 0, stream>>>(args);
    return hipGetLastError();
}

// r3d_clips_encode (a shard's padded model inputs from its raw pixel archive): blockIdx.y names a clip of the device-side table, the
// workgroup reads the clip's descriptor - and with it the camera row - once, by scalar loads (one address for the workgroup),
// decides on it before anything else, and each thread then encodes one output point (row, joint) from the clamped source frame
// through encode_point_f32, the routine the pre-pass itself writes with: the same bits, also in the padding rows.
extern "C" __global__ __launch_bounds__(256) void r3d_k_clips_encode(const ClipsEncArgs a) { clips_encode_body(a); }

// (ceil(max_rows * J / 256), num_clips) workgroups, one launch, nothing else
hipError_t launch_clips_encode(const ClipsEncArgs &args, int num_clips, hipStream_t stream) {
    const unsigned gx = (unsigned)((args.max_rows * args.J + 255) / 256);
    r3d_k_clips_encode<<<dim3(gx, (unsigned)num_clips), dim3(256), 0, stream>>>(args);
    return hipGetLastError();
}

// r3d_clips_repair (shard evaluation that survives dropped keypoints: the inputs r3d_clips_encode wrote, repaired in place before
// the first forward reads them), enqueued BEHIND r3d_clips_encode with the same table: one workgroup of 256 threads per (joint
// blockIdx.x, clip blockIdx.y).  It reads its descriptor by scalar loads and decides on it before anything else (clip_repair_clip of
// r3d_clips_repair.hpp).  Pass 1: the clip's rows in steps of 256, each thread judges one point (clip_repair_observed), each
// wavefront's ballot is one word of the clip-joint's bitmap of observed rows in LDS, stored by one lane; a barrier.  Pass 2, the
// same steps: a thread whose point is MISSING finds p - in the step's four words, else the running "last observed row in front of
// this step" every thread carries along, the same value in all of them - and q - in no more than max_gap / 64 + 2 words - with
// count-leading / trailing-zero operations and writes its own point of x, x_mirror and state through clip_repair_point, the routine
// the host hook runs.  Work per point is bounded whatever the pattern: no scan.  The counters are ballot popcounts, summed per
// wavefront, reduced through LDS and stored by one thread.  Observed points are never written and a missing point reads observed
// points only: in place, whatever the order.  Rows of one joint are J * F * 4 bytes apart: a wavefront's 64 points are 64 short
// accesses, served from the cache lines the other joints' workgroups of the clip read as well.  Nothing is pre-zeroed by the caller.
// At most 6 waves per SIMD: the body needs 38 VGPRs and would run 8, but the more workgroups a CU holds, the more clips' lines compete
// for the caches - on a 240-clip shard the launch takes 0.63 ms at 8 and at 7 waves and 0.56 ms at 6.
extern "C" __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 6))) void r3d_k_clips_repair(const ClipsRepairArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[CLIPS_REPAIR_LDS_BYTES];      // the bitmap (8 192 bytes), the per-wavefront words
    clips_repair_body(a, lds);
}

// (J, num_clips) workgroups of 256 threads, one launch, nothing else
hipError_t launch_clips_repair(const ClipsRepairArgs &args, int num_clips, hipStream_t stream) {
    static_assert(CLIPS_REPAIR_THREADS == 256, "the kernel's workgroups are 256 threads: a step is four bitmap words");
    r3d_k_clips_repair<<<dim3((unsigned)args.J, (unsigned)num_clips), dim3(CLIPS_REPAIR_THREADS), 0, stream>>>(args);
    return hipGetLastError();
}

// r3d_clips_poses (a shard's finished poses from what its forwards wrote): blockIdx.y names a clip of the r3d_clip_desc table, the
// workgroup reads the descriptor and the clip's raw_first by scalar loads and decides on them before anything else, and each thread
// finishes one output point (frame, joint) through pose_finish / pose_world of r3d_poses.hpp - the routines the host hook runs.  It
// is the elementwise end of a clip pass as r3d_clips_encode is its elementwise start: 12 or 24 bytes read and 12 and / or 24 written
// per thread, consecutive threads at consecutive addresses (the mirrored read is a permutation inside the row's J * 12 bytes).
extern "C" __global__ __launch_bounds__(256) void r3d_k_clips_poses(const ClipsPosesArgs a) { clips_poses_body(a); }

// (ceil(max_frames * J / 256), num_clips) workgroups, one launch, nothing else
hipError_t launch_clips_poses(const ClipsPosesArgs &args, int num_clips, hipStream_t stream) {
    const unsigned gx = (unsigned)((args.max_frames * args.J + 255) / 256);
    r3d_k_clips_poses<<<dim3(gx, (unsigned)num_clips), dim3(256), 0, stream>>>(args);
    return hipGetLastError();
}

// r3d_clips_project (a camera sweep's model inputs and ground truth from world poses): blockIdx.y names a (clip, camera) descriptor
// of the r3d_clip_project_desc table, the workgroup reads it by scalar loads - projection matrix, camera row, ground-truth
// transform - and decides on it before anything else, and each thread projects one output point (row, joint) from the clamped
// source frame through project_pixel of r3d_project.hpp, encodes the float64 pixel through encode_point_f32 - the routine the
// other two input paths write with - and, in the unpadded rows, writes the ground truth (pose_world), the pixel and its in-frame
// verdict: one integer atomicAdd per wavefront that saw a point outside.  12 bytes read and up to 12 + 12 + 12 + 16 written per
// thread, consecutive threads at consecutive addresses (the mirrored write is a permutation inside the row's J * 12 bytes).
extern "C" __global__ __launch_bounds__(256) void r3d_k_clips_project(const ClipsProjectArgs a) { clips_project_body(a); }

// (ceil(max_rows * J / 256), num_clips) workgroups, one launch, nothing else
hipError_t launch_clips_project(const ClipsProjectArgs &args, int num_clips, hipStream_t stream) {
    const unsigned gx = (unsigned)((args.max_rows * args.J + 255) / 256);
    r3d_k_clips_project<<<dim3(gx, (unsigned)num_clips), dim3(256), 0, stream>>>(args);
    return hipGetLastError();
}

// r3d_finalize_dev's pack (a handle's packed weights from device-resident state_dict tensors): a flat grid cut into runs of
// workgroups by a segment list in device memory (blockIdx.x finds its segment by bisection, uniformly), each thread one work item
// of r3d_pack.hpp - four consecutive columns of one output channel of one layer's image, or one bias - through pack_item, the
// routine the host replay (r3d_debug_pack_replay_host) runs.  One 16-byte store per thread, consecutive threads at consecutive
// addresses of the destination; the strided source rows go through the caches.
extern "C" __global__ __launch_bounds__(256) void r3d_k_pack(const PackArgs a) { pack_body(a); }

// one launch per phase (the layers' own images and biases; then the copies derived from them), `nblk` workgroups
hipError_t launch_pack(const PackArgs &args, int nblk, hipStream_t stream) {
    static_assert(PACK_THREADS == 256, "the kernel's workgroups are 256 threads");
    if (nblk <= 0) return hipSuccess;
    r3d_k_pack<<<dim3((unsigned)nblk), dim3(PACK_THREADS), 0, stream>>>(args);
    return hipGetLastError();
}

// r3d_clips_windows (a batch of materialised (RF, J, F) windows gathered from a pool of windows drawn from many clips): blockIdx.y
// names a window of the batch, the workgroup finds the run of the device-side table that holds it by bisection over win_first -
// uniformly, by scalar loads, as pack_body finds its segment - decides on that descriptor before anything else, and each thread
// copies one output point (row, joint) from the clamped source frame through window_point of r3d_windows.hpp, the routine the host
// hook runs.  8 or 12 bytes read and written per thread, consecutive threads at consecutive addresses on both sides except where
// the clamp repeats a frame (the mirrored read is a permutation inside the row's J * F * 4 bytes).
extern "C" __global__ __launch_bounds__(256) void r3d_k_clips_windows(const WindowsArgs a) { clips_windows_body(a); }

// (ceil(RF * J / 256), batch) workgroups, one launch, nothing else
hipError_t launch_clips_windows(const WindowsArgs &args, int batch, hipStream_t stream) {
    const unsigned gx = (unsigned)((args.RF * args.J + 255) / 256);
    r3d_k_clips_windows<<<dim3(gx, (unsigned)batch), dim3(256), 0, stream>>>(args);
    return hipGetLastError();
}

// r3d_streams_step (live streams lifted a frame at a time: a head and a ring of RF frames per stream in device memory) is two
// kernels, launched one behind the other.  r3d_k_streams_advance: one workgroup of one wavefront per stream; it reads the stream's
// head and action word - one address for the workgroup: scalar loads -, decides on them through stream_step of r3d_streams.hpp
// before anything else, has thread j put point j of the new frame into the ring slot (encode_point_f32, or a 32-bit copy), and
// thread 0 write the new head, emit and status.  r3d_k_streams_gather: blockIdx.y names a stream, the workgroup reads the head,
// emit and status the advance launch wrote - no launch writes a head that another of its workgroups reads -, and each thread copies
// one output point (row, joint) of the window from its ring slot through stream_gather_point, the routine the host hook runs: 8 or
// 12 bytes read and written per thread, consecutive threads at consecutive addresses of x; the ring is read in rows of J * F * 4
// bytes that wrap once.
extern "C" __global__ __launch_bounds__(64) void r3d_k_streams_advance(const StreamsArgs a) { streams_advance_body(a); }
extern "C" __global__ __launch_bounds__(256) void r3d_k_streams_gather(const StreamsArgs a) { streams_gather_body(a); }

// S workgroups of one wavefront advance the heads; then (ceil(RF * J / 256), S) workgroups gather the windows
hipError_t launch_streams_step(const StreamsArgs &args, hipStream_t stream) {
    r3d_k_streams_advance<<<dim3((unsigned)args.S), dim3(64), 0, stream>>>(args);
    if (const hipError_t err = hipGetLastError(); err != hipSuccess) return err;
    const unsigned gx = (unsigned)((args.RF * args.J + 255) / 256);
    r3d_k_streams_gather<<<dim3(gx, (unsigned)args.S), dim3(256), 0, stream>>>(args);
    return hipGetLastError();
}

// r3d_streams_poses (a live tick's finished poses: flip average, world transform and the re-projection residual against the
// keypoints that were fed in): one workgroup of one wavefront per stream; it reads the stream's emit and status words - one address
// for the workgroup: scalar loads - before anything else and returns unless the stream finished a frame this tick; then it reads
// the descriptor and the camera row (scalar loads again), thread j < J finishes joint j through pose_finish / pose_world /
// stream_reproj - the routines the host hook runs -, writes its outputs and parks its residual in LDS (17 doubles), and after a
// barrier thread 0 sums the J residuals in joint order and writes the two quality words.  S x J <= 17 threads of work per
// workgroup, a few hundred bytes per stream: the launch is LAUNCH-LATENCY-BOUND by construction - neither bandwidth nor occupancy
// nor the float64 divisions show in its time; it exists to replace a string of small torch launches by one.
extern "C" __global__ __launch_bounds__(64) void r3d_k_streams_poses(const StreamsPosesArgs a) { streams_poses_body(a); }

// S workgroups of one wavefront, one launch, nothing else
hipError_t launch_streams_poses(const StreamsPosesArgs &args, hipStream_t stream) {
    static_assert(STREAMS_POSES_THREADS == 64 && STREAMS_POSES_THREADS >= 17, "one wavefront holds a stream's joints");
    r3d_k_streams_poses<<<dim3((unsigned)args.S), dim3(STREAMS_POSES_THREADS), 0, stream>>>(args);
    return hipGetLastError();
}

// r3d_streams_repair (live streams that survive dropped keypoints: a repaired frame for r3d_streams_step to push, the ring entries
// a closing gap lets it improve, a per-stream track record), enqueued BEFORE the step of the same tick: one workgroup of one
// wavefront per stream; it reads the stream's head and action word - one address for the workgroup: scalar loads - and judges them
// through stream_step, the step's own routine, before anything else; a stream that takes no push has one thread write its word of
// `synthetic` and nothing more.  Otherwise thread j < J owns joint j through stream_repair_joint - the routine the host hook runs:
// it alone writes the joint's row of frame_out, its age and last, and the joint's entries of the ring, so no two threads touch the
// same word -, the wavefront's ballot of the joints not observed is the frame's mask, and thread 0 writes it and the word of
// `synthetic`.  A few hundred bytes per stream and, when a gap closes, at most RF - 1 ring entries of one joint:
// LAUNCH-LATENCY-BOUND by construction, as r3d_streams_poses is.
extern "C" __global__ __launch_bounds__(64) void r3d_k_streams_repair(const StreamsRepairArgs a) { streams_repair_body(a); }

// S workgroups of one wavefront, one launch, nothing else
hipError_t launch_streams_repair(const StreamsRepairArgs &args, hipStream_t stream) {
    static_assert(STREAMS_REPAIR_THREADS == 64 && STREAMS_REPAIR_THREADS >= 17, "one wavefront holds a stream's joints: its ballot is the mask");
    r3d_k_streams_repair<<<dim3((unsigned)args.S), dim3(STREAMS_REPAIR_THREADS), 0, stream>>>(args);
    return hipGetLastError();
}

// r3d_streams_peek (early poses for live streams of centred models: the windows a drain started now would emit, read out of the
// rings without ending the streams), enqueued AFTER the step of the same tick: blockIdx.y names a stream and blockIdx.z a look (the
// looks travel by value in the arguments), the workgroup reads the stream's head, action and status word - one address for the
// workgroup: scalar loads - and decides through stream_peek of r3d_streams_peek.hpp before anything is written, and each thread
// copies one output point (row, joint) through stream_peek_point, the gather's arithmetic with the preview frame in place of the
// emitted one and the routine the host hook runs: 8 or 12 bytes read and written per thread, consecutive threads at consecutive
// addresses of x.  The state is const to it.
extern "C" __global__ __launch_bounds__(256) void r3d_k_streams_peek(const StreamsPeekArgs a) { streams_peek_body(a); }

// (ceil(RF * J / 256), S, K) workgroups, one launch, nothing else
hipError_t launch_streams_peek(const StreamsPeekArgs &args, hipStream_t stream) {
    const unsigned gx = (unsigned)((args.RF * args.J + 255) / 256);
    r3d_k_streams_peek<<<dim3(gx, (unsigned)args.S, (unsigned)args.K), dim3(256), 0, stream>>>(args);
    return hipGetLastError();
}

// r3d_streams_assign (detections to live streams: per camera the association of a tick's unordered detections with the camera's
// stream slots, births and ends of tracks, and the action / frame / confidence rows r3d_streams_repair and r3d_streams_step read),
// enqueued BEFORE the repair / step of the same tick: one workgroup of one wavefront per camera.  Lane d owns detection d for the
// per-detection summary (its size and observed mask go to LDS, the valid bits are a ballot); the P x D pairs are dealt over the
// lanes, their cost keys - the bits of a non-negative double, which order as integers - go to LDS (at most 32 x 32 x 8 bytes; lane
// (d, half) owns column d's pairs with the slots of its parity: no division, one reference row per half wavefront and step); the
// greedy matching (stream_assign_greedy) is at most min(P, D) rounds, every lane ending with the same winner; the free slots are a
// ballot, and a free slot's popcount rank picks its detection; then lane p owns slot p: its state words and its row of every output
// through stream_assign_slot - the routine the host hook runs.  The state is read before the barrier in front of the matching and
// written after it, each slot's words by its own lane.
extern "C" __global__ __launch_bounds__(64) void r3d_k_streams_assign(const StreamsAssignArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[STREAMS_ASSIGN_LDS_BYTES];
    streams_assign_body(a, lds);
}

// C workgroups of one wavefront, one launch, nothing else
hipError_t launch_streams_assign(const StreamsAssignArgs &args, hipStream_t stream) {
    static_assert(STREAMS_ASSIGN_THREADS == 64, "one wavefront holds a camera's detections and slots: its ballots are their masks");
    r3d_k_streams_assign<<<dim3((unsigned)args.C), dim3(STREAMS_ASSIGN_THREADS), 0, stream>>>(args);
    return hipGetLastError();
}

// r3d_streams_link (one person across cameras: per scene the association of the cameras' tracks with a table of people by the
// distance of their world poses, births and ends of people, and the member table r3d_streams_fuse reads), enqueued between
// r3d_streams_poses and r3d_streams_fuse of the same tick: one workgroup of one wavefront per scene.  Lane g owns person g: its
// state words, its links and its row of the member table.  The cameras are visited in order, one uniform loop: lane g tests its
// link (stream_link_validate), P ballots find the held slots and drop a link a smaller g holds; lane p summarises slot p (its
// present mask goes to LDS, the candidate bits are a ballot); the G x P pairs are dealt over the lanes - lane (p, half) owns column
// p's pairs with the people of its parity -, their cost keys go to LDS at [g * P + p]; the greedy matching is r3d_streams_assign's
// (stream_assign_greedy); the free people are a ballot, and a free person's popcount rank picks its candidate.  A person born in
// camera c writes its reference pose to the state; the barrier that ends the camera's turn makes it visible to the lanes that form
// camera c + 1's keys.  Step C: lane g lists person g's finished members in LDS, lane (j, half) forms joint j of the people of its
// parity (stream_link_joint; the ballot is the person's new seen bits), then lane g finishes person g (stream_link_person).
extern "C" __global__ __launch_bounds__(64) void r3d_k_streams_link(const StreamsLinkArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[STREAMS_LINK_LDS_BYTES];
    streams_link_body(a, lds);
}

// N workgroups of one wavefront, one launch, nothing else
hipError_t launch_streams_link(const StreamsLinkArgs &args, hipStream_t stream) {
    static_assert(STREAMS_LINK_THREADS == 64, "one wavefront holds a scene's people and a camera's slots: its ballots are their masks");
    r3d_k_streams_link<<<dim3((unsigned)args.N), dim3(STREAMS_LINK_THREADS), 0, stream>>>(args);
    return hipGetLastError();
}

// r3d_streams_fuse (one world skeleton per person from several cameras: per group of streams and joint the gated, weighted mean of
// the world poses r3d_streams_poses wrote this tick), enqueued AFTER the r3d_streams_poses of the same tick: one workgroup of one
// wavefront per group; its M member words are one address per slot for the workgroup - scalar loads, read once, range-checked
// before they index anything -, thread j < J owns joint j through stream_fuse_joint - the routine the host hook runs -, which
// stages the candidates' points and weights in LDS (4 * 16 * 17 doubles, component-major so that the wavefront's threads touch
// consecutive doubles; each thread reads back only what it wrote itself: no barrier), runs the O(M^2) gate out of LDS and writes
// the joint's fused point, spread and count; the `used` word of slot m is the wavefront's ballot of "slot m was an inlier of my
// joint", written by thread 0, as r3d_streams_repair forms its mask.  At most 16 x 17 points per group: LAUNCH-LATENCY-BOUND by
// construction, as r3d_streams_poses is.
extern "C" __global__ __launch_bounds__(64) void r3d_k_streams_fuse(const StreamsFuseArgs a) {
    __shared__ double stage[STREAMS_FUSE_STAGE * STREAMS_FUSE_JOINTS];
    streams_fuse_body(a, stage);
}

// G workgroups of one wavefront, one launch, nothing else
hipError_t launch_streams_fuse(const StreamsFuseArgs &args, hipStream_t stream) {
    static_assert(STREAMS_FUSE_THREADS == 64 && STREAMS_FUSE_THREADS >= STREAMS_FUSE_JOINTS, "one wavefront holds a group's joints: its ballots are the used words");
    r3d_k_streams_fuse<<<dim3((unsigned)args.G), dim3(STREAMS_FUSE_THREADS), 0, stream>>>(args);
    return hipGetLastError();
}

}  // namespace r3d
