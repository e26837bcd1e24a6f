// Speed of live plate tracks on a calibrated ground plane, with an alert over a limit: lp_speed_update (include/lp_hip.h).  The
// tracker says which plate, lp_zone_update which way and how long, both in pixels of the frame; this maps the tracker's anchor through a
// per-stream homography to millimetres on a plane and differences the positions over time.  The reference has nothing here; the
// written-down specification is yolov6/utils/speed.py (SpeedNp), which this file matches on every int32 of the three outputs and of the
// memo (tests/test_speed_gpu.py).
//
// One kernel, one workgroup of 128 threads per stream, lane t = slot t; the tracker state is read as lp_track_update left it (layout:
// lp_streams.h) and never written; the phases c and d are the shared pieces of lp_track_read.inc.
//   a. the stream's 32 map words are staged in LDS once;
//   b. lane t reads slot t's first 16 bytes (id, first, last, hits) and its memo header (64 bytes), and of a line that holds samples the
//      newest one (16 bytes: the row of step 7 and the event of step 2 carry its position).  Only an eligible slot with a new detection
//      reads its box; only a lane that pushes stores a sample (16 bytes), and only it reads the oldest one.  It settles steps 2 to 6 in
//      registers and writes its row.  The world point is fp64, one rounded operation at a time (the file is compiled with
//      -ffp-contract=off and says so again below), with two plain divisions; everything behind it is integer, the root exact: a
//      double-precision estimate corrected by integer compares;
//   c. only a slot that emits an alert (kind 1) has its votes read: rule 8 by track_read_head, one (slot, head) per thread and round, as
//      step c of lp_zones.hip;
//   d. the events are numbered in slot order by a prefix sum of the counts (a shuffle scan per wave, the two waves joined in LDS) and
//      written by their lane, three 16-byte stores a line; lines at or past max_events are not written, the lines from the count to
//      max_events are zeroed by all lanes.
// All stores are ordinary vector stores from plain C++; no atomics, no workspace.
#include "lp_internal.h"
#include "lp_streams.h"
#include "lp_track_read.inc"

#pragma clang fp contract(off)

namespace lp {

namespace {

constexpr int SP_T = TR_SLOTS;                  // threads of the workgroup: one per slot
constexpr int SP_MAP = LP_SPEED_MAP_WORDS, SP_MEMO = LP_SPEED_MEMO_WORDS, SP_RING = LP_SPEED_RING;
constexpr int SP_ROW_COLS = 8, SP_EV_COLS = 12;
constexpr int SP_MAP_PERIOD = 18, SP_MAP_LIMIT = 19, SP_MAP_GAP = 20, SP_MAP_SPAN = 21, SP_MAP_ENABLED = 22;
constexpr int SP_MAX_CONFIRM = 65535, SP_I32_MAX = 0x7FFFFFFF;
static_assert(SP_T == 128 && SP_MAP == 32 && SP_MEMO == 48 && SP_RING == 8 && SP_MEMO == 16 + 4 * SP_RING, "lp_speed.hip: the layouts of lp_hip.h");
enum { SK_ALERT = 1, SK_ENDED = 3 };

struct SpeedEst { int speed, vx, vy, span_ms; };

typedef unsigned long long u64;
typedef long long i64;

__device__ __forceinline__ i64 sjoin(int lo, int hi) { return (i64)(((u64)(unsigned)hi << 32) | (u64)(unsigned)lo); }
__device__ __forceinline__ i64 ssub(i64 a, i64 b) { return (i64)((u64)a - (u64)b); }                 // wraps

// floor(sqrt(d2)), exact, for d2 <= 2^63: the double root is within a few units of it, integer compares settle it
__device__ __forceinline__ u64 sroot(u64 d2) {
    u64 s = (u64)__dsqrt_rn((double)d2);                                                // at most 3037000500: s * s and (s + 1)^2 fit
    while (s * s > d2) --s;
    while ((s + 1) * (s + 1) <= d2) ++s;
    return s;
}

__device__ __forceinline__ int sdiv_clamp(u64 num, u64 dt) {
    const u64 q = num / dt;
    return q > (u64)SP_I32_MAX ? SP_I32_MAX : (int)q;
}

// step 5 of the rule for differences in mm (|dx|, |dy| <= 2^31) and dt > 0 in microseconds
__device__ __forceinline__ SpeedEst sestimate(i64 dx, i64 dy, i64 dt) {
    const u64 ax = (u64)(dx < 0 ? -dx : dx), ay = (u64)(dy < 0 ? -dy : dy), t = (u64)dt;
    const u64 s = sroot(ax * ax + ay * ay);
    SpeedEst e;
    e.speed = sdiv_clamp(s * 1000000ull, t);
    const int vx = sdiv_clamp(ax * 1000000ull, t), vy = sdiv_clamp(ay * 1000000ull, t);
    e.vx = dx < 0 ? -vx : vx;
    e.vy = dy < 0 ? -vy : vy;
    const u64 ms = t / 1000ull;
    e.span_ms = ms > (u64)SP_I32_MAX ? SP_I32_MAX : (int)ms;
    return e;
}

// grid (n_streams), block (128)
__global__ __launch_bounds__(SP_T) void speed_kernel(const int* __restrict__ state, int T, long long sstride, const TrackNcls ncls,
                                                     const int* __restrict__ map, const long long* __restrict__ clock, int min_hits, int confirm,
                                                     int32_t* __restrict__ memo, int32_t* __restrict__ speed_i, int32_t* __restrict__ speed_ev,
                                                     int32_t* __restrict__ speed_count, int max_events) {
    __shared__ int s_map[SP_MAP];
    __shared__ int s_wsum[2], s_need[SP_T], s_best[SP_T * TR_HEADS];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- a. the map ----------------------------------------------------------------------------------------------------------------
    if (tid < SP_MAP) s_map[tid] = map[(long long)s * SP_MAP + tid];
    __syncthreads();
    const bool enabled = s_map[SP_MAP_ENABLED] != 0;
    const int* const hdr = state + (long long)s * sstride;
    const int* const sl = hdr + TR_HDR_WORDS + (long long)tid * TR_SLOT_WORDS;           // read for tid < T only
    const int now = hdr[0];                                                             // the stream's frame counter
    // ---- b. steps 1 to 7 of slot tid -------------------------------------------------------------------------------------------------
    int4 h = make_int4(0, 0, 0, 0);
    int ev_kind = 0;
    int4 ev0 = make_int4(0, 0, 0, 0), ev1 = ev0, ev2 = ev0;                             // the event's line, the key still missing
    if (tid < T) {
        h = *(const int4*)sl;                                                           // id, first, last, hits
        int4* const ml = (int4*)(memo + ((long long)s * T + tid) * SP_MEMO);            // (s * T + tid + 1) * 48 <= the memo's words
        int4 m0 = ml[0], m1 = ml[1], m2 = ml[2], m3 = ml[3];                            // id + 1, last, pushed, head | first | speed, vx, vy, peak | over, span
        const int4 zero = make_int4(0, 0, 0, 0);
        const bool eligible = enabled && h.w > 0 && h.w >= min_hits;                    // 1
        const int idp1 = (int)((unsigned)h.x + 1u);
        bool have = m0.x != 0;
        int4 newest = zero;
        if (have && m0.z > 0) newest = ml[4 + ((m0.w - 1) & (SP_RING - 1))];
        if (have && (!eligible || m0.x != idp1)) {                                      // 2
            if (m0.z >= 2) {
                const i64 dt = ssub(sjoin(newest.x, newest.y), sjoin(m1.x, m1.y));
                int aux = 0;
                if (dt > 0) aux = sestimate((i64)newest.z - (i64)m1.z, (i64)newest.w - (i64)m1.w, dt).speed;
                ev_kind = SK_ENDED;
                ev0 = make_int4(SK_ENDED, 0, wrap_diff(m0.x, 1), tid);
                ev1 = make_int4(m0.y, m2.w, newest.z, newest.w);
                ev2 = make_int4(0, 0, 0, aux);
            }
#pragma unroll
            for (int q = 0; q < SP_MEMO / 4; ++q) ml[q] = zero;
            have = false;
            m0 = m1 = m2 = m3 = newest = zero;
        }
        int4 r0 = make_int4(-1, 0, 0, 0), r1 = zero;
        if (eligible) {
            bool fresh = false, estimated = false, touched = false;
            if (!have) {                                                                // 3
                m0.x = idp1;
                m2.x = -1;
            }
            if (!have || h.z != m0.y) {                                                 // 3, 4: a new detection
                touched = true;
                m0.y = h.z;
                const float4 box = *(const float4*)(sl + TR_W_BOX);
                const float ax = (box.x + box.z) * 0.5f, ay = (box.y + box.w) * 0.5f;
                const double x = (double)ax, y = (double)ay;
                double hh[9];
#pragma unroll
                for (int q = 0; q < 9; ++q) hh[q] = __hiloint2double(s_map[2 * q + 1], s_map[2 * q]);
                const double u0 = hh[0] * x, u1 = hh[1] * y, u2 = u0 + u1, u = u2 + hh[2];
                const double v0 = hh[3] * x, v1 = hh[4] * y, v2 = v0 + v1, v = v2 + hh[5];
                const double w0 = hh[6] * x, w1 = hh[7] * y, w2 = w0 + w1, w = w2 + hh[8];
                const double X = u / w, Y = v / w;
                const double px = X * 1000.0, py = Y * 1000.0;
                const bool valid = finite_pair(ax, ay) && w > 0.0 && fabs(px) <= 1073741824.0 && fabs(py) <= 1073741824.0;
                if (valid) {
                    const i64 period = (i64)s_map[SP_MAP_PERIOD];
                    const i64 base = clock ? (i64)clock[s] : (i64)((u64)(i64)now * (u64)period);
                    const i64 tt = ssub(base, (i64)((u64)(i64)wrap_diff(now, h.z) * (u64)period));
                    if (m0.z == 0 || ssub(tt, sjoin(newest.x, newest.y)) >= (i64)s_map[SP_MAP_GAP]) {
                        newest = make_int4((int)(unsigned)((u64)tt & 0xFFFFFFFFull), (int)(unsigned)((u64)tt >> 32), (int)rint(px), (int)rint(py));
                        if (m0.z == 0) m1 = newest;
                        const int head = m0.w & (SP_RING - 1);
                        ml[4 + head] = newest;
                        m0.w = (head + 1) & (SP_RING - 1);
                        m0.z = m0.z == SP_I32_MAX ? SP_I32_MAX : m0.z + 1;
                        fresh = true;
                    }
                }
            }
            const int n = m0.z < SP_RING ? m0.z : SP_RING;
            if (fresh && n >= 2) {                                                      // 5
                const int4 o = ml[4 + (m0.z >= SP_RING ? m0.w : 0)];                    // never the sample just stored: n >= 2
                const i64 dt = ssub(sjoin(newest.x, newest.y), sjoin(o.x, o.y));
                if (dt >= (i64)s_map[SP_MAP_SPAN]) {                                    // min_span_us >= 1: dt > 0
                    const SpeedEst e = sestimate((i64)newest.z - (i64)o.z, (i64)newest.w - (i64)o.w, dt);
                    m2.x = e.speed; m2.y = e.vx; m2.z = e.vy;
                    m2.w = m2.w > e.speed ? m2.w : e.speed;
                    m3.y = e.span_ms;
                    estimated = true;
                }
            }
            int over = m3.x & 0xFFFF, alerted = (m3.x >> 16) & 1;
            const int limit = s_map[SP_MAP_LIMIT];
            if (estimated && limit > 0) {                                               // 6
                if (m2.x > limit) {
                    over = over < SP_MAX_CONFIRM ? over + 1 : SP_MAX_CONFIRM;
                    if (over >= confirm && !alerted) {
                        alerted = 1;
                        ev_kind = SK_ALERT;                                             // (a line that was gone has one sample: no estimate)
                        ev0 = make_int4(SK_ALERT, 0, h.x, tid);
                        ev1 = make_int4(h.z, m2.x, newest.z, newest.w);
                        ev2 = make_int4(0, 0, h.w, limit);
                    }
                } else {
                    over = 0;
                }
                m3.x = over | alerted << 16;
            }
            if (touched) { ml[0] = m0; ml[1] = m1; ml[2] = m2; ml[3] = m3; }
            r0 = make_int4(h.x, m2.x, m2.y, m2.z);                                      // 7
            r1 = make_int4(n ? newest.z : 0, n ? newest.w : 0, m3.y, n | (fresh ? 1 << 8 : 0) | alerted << 9);
        }
        int4* const row = (int4*)(speed_i + ((long long)s * T + tid) * SP_ROW_COLS);
        row[0] = r0;
        row[1] = r1;
    }
    const int cnt = ev_kind != 0 ? 1 : 0;
    s_need[tid] = ev_kind == SK_ALERT ? 1 : 0;
    // ---- d. (first half) the events numbered in slot order ---------------------------------------------------------------------------
    const int incl = wave_inclusive_sum(cnt, lane, wave, s_wsum);
    __syncthreads();
    // ---- c. rule 8 for the slots that alert --------------------------------------------------------------------------------------------
    read_needed_heads<SP_T>(hdr + TR_HDR_WORDS, T, ncls, s_need, s_best);
    __syncthreads();
    // ---- d. the event lines, written by their lane -------------------------------------------------------------------------------------
    const int total = s_wsum[0] + s_wsum[1];
    int32_t* const ev = speed_ev + (long long)s * max_events * SP_EV_COLS;               // line k < max_events only
    const int k = events_before(incl, cnt, wave, s_wsum);
    if (cnt > 0 && k < max_events) {
        if (ev_kind == SK_ALERT) {
            unsigned klo, khi;
            pack_key(s_best + tid * TR_HEADS, klo, khi);
            ev2.x = (int)klo;
            ev2.y = (int)khi;
        }
        int4* const o = (int4*)(ev + (long long)k * SP_EV_COLS);
        o[0] = ev0;
        o[1] = ev1;
        o[2] = ev2;
    }
    close_event_list<SP_T, SP_EV_COLS>(ev, total, max_events, speed_count + s);
}

// the dimensions of a call, the state within an int32 index
std::string speed_dims_fault(int n_streams, int max_tracks) {
    return stream_words_fault(n_streams, max_tracks, {track_state_stride(max_tracks)}, "a state of fewer than 2^31 words");
}

}  // namespace

}  // namespace lp

using namespace lp;

extern "C" size_t lp_speed_state_bytes(int n_streams, int max_tracks) {
    if (!speed_dims_fault(n_streams, max_tracks).empty()) return 0;
    return (size_t)n_streams * (size_t)max_tracks * SP_MEMO * 4;
}

extern "C" int lp_speed_update(const void* track_state, int n_streams, int max_tracks, const int* ncls, const void* ground_map, const void* clock_us,
                               int min_hits, int confirm, void* memo, void* speed_i, void* speed_ev, void* speed_count, int max_events, void* stream) {
    const std::string fn = "lp_speed_update: ";
    TrackNcls nc;
    std::string why = speed_dims_fault(n_streams, max_tracks);
    if (why.empty()) why = max_events_fault(n_streams, max_events, SP_EV_COLS);
    if (why.empty()) why = ncls_fault(ncls, nc);
    if (why.empty()) why = min_hits_fault(min_hits);
    if (!why.empty()) return fail(LP_ERR_ARG, fn + why);
    if (confirm < 1 || confirm > SP_MAX_CONFIRM) return fail(LP_ERR_ARG, fn + "confirm must be in 1.." + std::to_string(SP_MAX_CONFIRM));
    if (!track_state || !ground_map || !memo || !speed_i || (max_events > 0 && !speed_ev) || !speed_count) return fail(LP_ERR_ARG, fn + "null pointer");
    if ((((uintptr_t)track_state | (uintptr_t)ground_map | (uintptr_t)memo | (uintptr_t)speed_i | (uintptr_t)speed_ev | (uintptr_t)speed_count) & 15) != 0 ||
        ((uintptr_t)clock_us & 7) != 0)
        return fail(LP_ERR_ARG, fn + "the tracker state, the map, the memo and the three outputs must be 16-byte aligned, the clock 8-byte aligned");
    const long long sstride = track_state_stride(max_tracks);
    {   // no buffer that is written may overlap the state, the map, the clock or another one
        const Region reg[] = {{track_state, (size_t)n_streams * (size_t)sstride * 4, false},
                              {ground_map, (size_t)n_streams * SP_MAP * 4, false},
                              {clock_us, clock_us ? (size_t)n_streams * 8 : 0, false},
                              {memo, (size_t)n_streams * (size_t)max_tracks * SP_MEMO * 4, true},
                              {speed_i, (size_t)n_streams * (size_t)max_tracks * SP_ROW_COLS * 4, true},
                              {speed_ev, (size_t)n_streams * (size_t)max_events * SP_EV_COLS * 4, true},
                              {speed_count, (size_t)n_streams * 4, true}};
        if (regions_clash(reg, (int)(sizeof(reg) / sizeof(reg[0]))))
            return fail(LP_ERR_ARG, fn + "the memo and the three outputs may overlap neither the state, the map, the clock nor each other");
    }
    hipLaunchKernelGGL(speed_kernel, dim3((unsigned)n_streams), dim3(SP_T), 0, (hipStream_t)stream, (const int*)track_state, max_tracks, sstride, nc,
                       (const int*)ground_map, (const long long*)clock_us, min_hits, confirm, (int32_t*)memo, (int32_t*)speed_i, (int32_t*)speed_ev,
                       (int32_t*)speed_count, max_events);
    LP_HIP_CHECK(hipGetLastError());
    return LP_OK;
}
