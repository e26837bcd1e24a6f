// Tripwires and zones on live plate tracks: lp_zone_update (include/lp_hip.h).  The tracker, the watchlists and the sightings log say
// which plate; a gate, a car park or a street also asks which way it went and how long it has been there.  The reference has nothing
// here; the written-down specification is yolov6/utils/zones.py (ZoneEventsNp), which this file matches on every int32 of the four
// outputs and of the memo (tests/test_zones_gpu.py).
//
// One kernel, one workgroup of 128 threads per stream, lane t = slot t; the tracker state is read as lp_track_update left it (layout:
// lp_streams.h) and never written; the phases c and d and the close of e are the shared pieces of lp_track_read.inc.
//   a. the stream's packed geometry (LP_ZONE_MAP_WORDS words) is staged in LDS once;
//   b. lane t reads slot t's first 16 bytes (id, first, last, hits), its memo line and, if the slot is eligible, its box.  It settles
//      steps 2 to 5 of the rule in registers: the zones a track that is gone ended in, the two masks of crossed lines, the masks of
//      entered, left and alerted zones; it counts its events, writes its memo line and adds to the occupancy and the totals in LDS
//      (integer atomics: the order does not matter).  The geometry is fp64, one rounded subtract or multiply at a time (the file is
//      compiled with -ffp-contract=off and says so again below);
//   c. only a slot that emits an event of kind 1 to 4 has its votes read: rule 8 by track_read_head, one (slot, head) per thread and
//      round, as live_gather_kernel of lp_watch_live.hip does;
//   d. the events are numbered in slot order by a prefix sum of the counts (a shuffle scan per wave, the two waves joined in LDS)
//      and written by their lane, three 16-byte stores a line; lines at or past max_events are not written, the lines from the count
//      to max_events are zeroed by all lanes;
//   e. zone_count, zone_occ, the totals (memo rows T and T + 1, copied to zone_totals).
// All stores are ordinary vector stores from plain C++.
#include "lp_internal.h"
#include "lp_streams.h"
#include "lp_track_read.inc"

#pragma clang fp contract(off)

namespace lp {

namespace {

constexpr int ZN_T = TR_SLOTS;                  // threads of the workgroup: one per slot
constexpr int ZN_LINES = LP_ZONE_MAX_LINES, ZN_ZONES = LP_ZONE_MAX_ZONES, ZN_VERTS = LP_ZONE_MAX_VERTS;
constexpr int ZN_MEMO_WORDS = 16, ZN_EV_COLS = 12;
constexpr int ZN_MAP_LINES = 16, ZN_MAP_ZHDR = ZN_MAP_LINES + 4 * ZN_LINES, ZN_MAP_VERTS = ZN_MAP_ZHDR + 4 * ZN_ZONES;
constexpr int ZN_MAP_WORDS = ZN_MAP_VERTS + ZN_ZONES * ZN_VERTS * 2;
static_assert(ZN_MAP_WORDS == LP_ZONE_MAP_WORDS && ZN_T == 128 && ZN_LINES == 16 && ZN_ZONES == 8, "lp_zones.hip: the packed map of lp_hip.h");
enum { ZK_CROSS = 1, ZK_ENTER = 2, ZK_LEFT = 3, ZK_DWELL = 4, ZK_ENDED = 5 };

// cross(P, Q, R) = (Qx - Px) * (Ry - Py) - (Qy - Py) * (Rx - Px), every operation rounded on its own
__device__ __forceinline__ double zcross(double px, double py, double qx, double qy, double rx, double ry) {
    const double a = (qx - px) * (ry - py);
    const double b = (qy - py) * (rx - px);
    return a - b;
}

__device__ __forceinline__ int zclamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__device__ __forceinline__ void zstore_event(int32_t* __restrict__ line, int kind, int index, int id, int slot, int frame, int value, int axb, int ayb,
                                             int klo, int khi, int hits) {
    int4* o = (int4*)line;
    o[0] = make_int4(kind, index, id, slot);
    o[1] = make_int4(frame, value, axb, ayb);
    o[2] = make_int4(klo, khi, hits, 0);
}

// grid (n_streams), block (128)
__global__ __launch_bounds__(ZN_T) void zone_kernel(const int* __restrict__ state, int T, long long sstride, const TrackNcls ncls,
                                                    const int* __restrict__ map, int min_hits, int32_t* __restrict__ memo,
                                                    int32_t* __restrict__ zone_ev, int32_t* __restrict__ zone_count, int max_events,
                                                    int32_t* __restrict__ zone_occ, int32_t* __restrict__ zone_totals) {
    __shared__ int s_map[ZN_MAP_WORDS];
    __shared__ int s_occ[ZN_ZONES], s_tot[2 * ZN_LINES], s_wsum[2], s_need[ZN_T], s_best[ZN_T * TR_HEADS];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- a. the geometry ---------------------------------------------------------------------------------------------------------
    for (int i = tid; i < ZN_MAP_WORDS; i += ZN_T) s_map[i] = map[(long long)s * ZN_MAP_WORDS + i];
    if (tid < ZN_ZONES) s_occ[tid] = 0;
    if (tid < 2 * ZN_LINES) s_tot[tid] = 0;
    __syncthreads();
    const int nl = zclamp(s_map[0], ZN_LINES), nz = zclamp(s_map[1], ZN_ZONES);
    const int* const hdr = state + (long long)s * sstride;
    const int* const sl = hdr + TR_HDR_WORDS + (long long)tid * TR_SLOT_WORDS;           // read for tid < T only
    int32_t* const mbase = memo + (long long)s * (T + 2) * ZN_MEMO_WORDS;                // (s + 1) * (T + 2) * 16 <= the memo's words
    const int now = hdr[0];                                                             // the stream's frame counter
    // ---- b. steps 1 to 5 of slot tid ------------------------------------------------------------------------------------------------
    int4 h = make_int4(0, 0, 0, 0);
    int gone_mask = 0, gone_id = 0, gone_last = 0, gone_ax = 0, gone_ay = 0, gone_enter[ZN_ZONES];
    int enter[ZN_ZONES], axb = 0, ayb = 0;
    unsigned up = 0, down = 0, entered = 0, left = 0, alert = 0;
    int cnt = 0;
#pragma unroll
    for (int z = 0; z < ZN_ZONES; ++z) gone_enter[z] = enter[z] = 0;
    if (tid < T) {
        h = *(const int4*)sl;                                                           // id, first, last, hits
        int4* const ml = (int4*)(mbase + tid * ZN_MEMO_WORDS);
        const int4 m0 = ml[0], m1 = ml[1], m2 = ml[2], m3 = ml[3];
        const bool eligible = h.w > 0 && h.w >= min_hits;                               // 1
        bool have = m0.x != 0;
        const int m_enter[ZN_ZONES] = {m1.y, m1.z, m1.w, m2.x, m2.y, m2.z, m2.w, m3.x};
        if (have && (!eligible || m0.x != h.x + 1)) {                                   // 2
            gone_mask = m1.x & 0xFF;
            gone_id = m0.x - 1; gone_last = m0.y; gone_ax = m0.z; gone_ay = m0.w;
#pragma unroll
            for (int z = 0; z < ZN_ZONES; ++z) gone_enter[z] = m_enter[z];
            cnt += __popc(gone_mask);
            have = false;
            if (!eligible) {
                const int4 zero = make_int4(0, 0, 0, 0);
                ml[0] = zero; ml[1] = zero; ml[2] = zero; ml[3] = zero;
            }
        }
        if (eligible) {
            const float4 box = *(const float4*)(sl + TR_W_BOX);
            const float ax = (box.x + box.z) * 0.5f, ay = (box.y + box.w) * 0.5f;
            axb = __float_as_int(ax); ayb = __float_as_int(ay);
            const bool fin = finite_pair(ax, ay);
            const double px = (double)ax, py = (double)ay;
            unsigned old_inside = 0, alerted = 0, inside = 0;
            if (have) {
                old_inside = (unsigned)m1.x & 0xFFu;
                alerted = ((unsigned)m1.x >> 8) & 0xFFu;
#pragma unroll
                for (int z = 0; z < ZN_ZONES; ++z) enter[z] = m_enter[z];
                const float ox = __int_as_float(m0.z), oy = __int_as_float(m0.w);
                if (fin && finite_pair(ox, oy)) {                                       // 4: the lines
                    const double p0x = (double)ox, p0y = (double)oy;
                    for (int l = 0; l < nl; ++l) {
                        const float* g = (const float*)(s_map + ZN_MAP_LINES + 4 * l);
                        const double lax = (double)g[0], lay = (double)g[1], lbx = (double)g[2], lby = (double)g[3];
                        const double d0 = zcross(lax, lay, lbx, lby, p0x, p0y), d1 = zcross(lax, lay, lbx, lby, px, py);
                        const double e0 = zcross(p0x, p0y, px, py, lax, lay), e1 = zcross(p0x, p0y, px, py, lbx, lby);
                        const bool between = (e0 <= 0.0 && e1 > 0.0) || (e0 > 0.0 && e1 <= 0.0);
                        if (between && d0 <= 0.0 && d1 > 0.0) up |= 1u << l;
                        if (between && d0 > 0.0 && d1 <= 0.0) down |= 1u << l;
                    }
                }
            }
            if (fin) {                                                                  // inside: the crossing number
                for (int z = 0; z < nz; ++z) {
                    const int n = zclamp(s_map[ZN_MAP_ZHDR + 4 * z], ZN_VERTS);
                    const float* v = (const float*)(s_map + ZN_MAP_VERTS + 2 * ZN_VERTS * z);
                    unsigned par = 0;
                    for (int i = 0; i < n; ++i) {
                        const int j = i + 1 == n ? 0 : i + 1;
                        const double xi = (double)v[2 * i], yi = (double)v[2 * i + 1], xj = (double)v[2 * j], yj = (double)v[2 * j + 1];
                        if ((yi > py) != (yj > py)) {
                            const double a = (xj - xi) * (py - yi);
                            const double b = (px - xi) * (yj - yi);
                            const double t = a - b;
                            if (yj > yi ? t > 0.0 : t < 0.0) par ^= 1u;
                        }
                    }
                    inside |= par << z;
                }
            }
#pragma unroll
            for (int z = 0; z < ZN_ZONES; ++z) {                                        // 3, 4: the transitions; 5: the dwell alerts
                const unsigned bit = 1u << z;
                if (z < nz) {
                    if ((inside & bit) && !(old_inside & bit)) {
                        enter[z] = h.z;
                        alerted &= ~bit;
                        entered |= bit;
                    } else if ((old_inside & bit) && !(inside & bit)) {
                        left |= bit;
                    }
                    const int dwell = s_map[ZN_MAP_ZHDR + 4 * z + 1];
                    if ((inside & bit) && dwell > 0 && !(alerted & bit) && wrap_diff(now, enter[z]) >= dwell) {
                        alert |= bit;
                        alerted |= bit;
                    }
                    if (inside & bit) atomicAdd(&s_occ[z], 1);
                }
            }
            cnt += __popc(up) + __popc(down) + __popc(entered) + __popc(left) + __popc(alert);
            for (unsigned m = up; m; m &= m - 1) atomicAdd(&s_tot[__ffs(m) - 1], 1);
            for (unsigned m = down; m; m &= m - 1) atomicAdd(&s_tot[ZN_LINES + __ffs(m) - 1], 1);
            ml[0] = make_int4(h.x + 1, h.z, axb, ayb);
            ml[1] = make_int4((int)(inside | alerted << 8), enter[0], enter[1], enter[2]);
            ml[2] = make_int4(enter[3], enter[4], enter[5], enter[6]);
            ml[3] = make_int4(enter[7], 0, 0, 0);
        }
    }
    const bool need = (up | down | entered | left | alert) != 0;
    s_need[tid] = need ? 1 : 0;
    // ---- d. (first half) the events numbered in slot order -----------------------------------------------------------------------
    const int incl = wave_inclusive_sum(cnt, lane, wave, s_wsum);
    __syncthreads();
    // ---- c. rule 8 for the slots that emit a kind 1 to 4 event ----------------------------------------------------------------------
    read_needed_heads<ZN_T>(hdr + TR_HDR_WORDS, T, ncls, s_need, s_best);
    __syncthreads();
    // ---- d. the event lines, written by their lane ---------------------------------------------------------------------------------
    const int total = s_wsum[0] + s_wsum[1];
    int32_t* const ev = zone_ev + (long long)s * max_events * ZN_EV_COLS;                // line k < max_events only
    int k = events_before(incl, cnt, wave, s_wsum);
    if (cnt > 0) {
        for (unsigned m = (unsigned)gone_mask; m; m &= m - 1) {
            const int z = __ffs(m) - 1;
            int ef = 0;
#pragma unroll
            for (int q = 0; q < ZN_ZONES; ++q) ef = q == z ? gone_enter[q] : ef;
            if (k < max_events) zstore_event(ev + (long long)k * ZN_EV_COLS, ZK_ENDED, z, gone_id, tid, gone_last, wrap_diff(gone_last, ef), gone_ax, gone_ay, 0, 0, 0);
            ++k;
        }
        if (need) {
            unsigned klo, khi;
            pack_key(s_best + tid * TR_HEADS, klo, khi);
            for (int l = 0; l < ZN_LINES; ++l) {
                const int dir = (int)((up >> l) & 1u) - (int)((down >> l) & 1u);
                if (dir != 0) {
                    if (k < max_events) zstore_event(ev + (long long)k * ZN_EV_COLS, ZK_CROSS, l, h.x, tid, h.z, dir, axb, ayb, (int)klo, (int)khi, h.w);
                    ++k;
                }
            }
#pragma unroll
            for (int z = 0; z < ZN_ZONES; ++z) {
                const unsigned bit = 1u << z;
                if ((entered | left) & bit) {
                    const bool in = (entered & bit) != 0;
                    if (k < max_events)
                        zstore_event(ev + (long long)k * ZN_EV_COLS, in ? ZK_ENTER : ZK_LEFT, z, h.x, tid, h.z, in ? 0 : wrap_diff(h.z, enter[z]), axb, ayb, (int)klo,
                                     (int)khi, h.w);
                    ++k;
                }
                if (alert & bit) {
                    if (k < max_events)
                        zstore_event(ev + (long long)k * ZN_EV_COLS, ZK_DWELL, z, h.x, tid, h.z, wrap_diff(now, enter[z]), axb, ayb, (int)klo, (int)khi, h.w);
                    ++k;
                }
            }
        }
    }
    // ---- e. the count, the occupancy, the totals ------------------------------------------------------------------------------------
    close_event_list<ZN_T, ZN_EV_COLS>(ev, total, max_events, zone_count + s);
    if (tid < ZN_ZONES) zone_occ[(long long)s * ZN_ZONES + tid] = s_occ[tid];
    if (tid < 2 * ZN_LINES) {
        int32_t* const row = mbase + (long long)(T + (tid >> 4)) * ZN_MEMO_WORDS + (tid & 15);
        const int v = (int)((unsigned)*row + (unsigned)s_tot[tid]);
        *row = v;
        zone_totals[(long long)s * 2 * ZN_LINES + tid] = v;
    }
}

// the dimensions of a call, the state and the map within an int32 index
std::string zone_dims_fault(int n_streams, int max_tracks) {
    return stream_words_fault(n_streams, max_tracks, {track_state_stride(max_tracks), ZN_MAP_WORDS}, "a state and a map of fewer than 2^31 words");
}

}  // namespace

}  // namespace lp

using namespace lp;

extern "C" size_t lp_zone_state_bytes(int n_streams, int max_tracks) {
    if (!zone_dims_fault(n_streams, max_tracks).empty()) return 0;
    return (size_t)n_streams * (size_t)(max_tracks + 2) * ZN_MEMO_WORDS * 4;
}

extern "C" int lp_zone_update(const void* track_state, int n_streams, int max_tracks, const int* ncls, const void* zone_map, int min_hits,
                              int32_t* memo, int32_t* zone_ev, int32_t* zone_count, int max_events, int32_t* zone_occ, int32_t* zone_totals,
                              void* stream) {
    const std::string fn = "lp_zone_update: ";
    TrackNcls nc;
    std::string why = zone_dims_fault(n_streams, max_tracks);
    if (why.empty()) why = max_events_fault(n_streams, max_events, ZN_EV_COLS);
    if (why.empty()) why = ncls_fault(ncls, nc);
    if (why.empty()) why = min_hits_fault(min_hits);
    if (!why.empty()) return fail(LP_ERR_ARG, fn + why);
    if (!track_state || !zone_map || !memo || (max_events > 0 && !zone_ev) || !zone_count || !zone_occ || !zone_totals)
        return fail(LP_ERR_ARG, fn + "null pointer");
    if ((((uintptr_t)track_state | (uintptr_t)zone_map | (uintptr_t)memo | (uintptr_t)zone_ev | (uintptr_t)zone_count | (uintptr_t)zone_occ |
          (uintptr_t)zone_totals) & 15) != 0)
        return fail(LP_ERR_ARG, fn + "the tracker state, the map, the memo and the four outputs must be 16-byte aligned");
    const long long sstride = track_state_stride(max_tracks);
    {   // no buffer that is written may overlap the state, the map or another one
        const Region reg[] = {{track_state, (size_t)n_streams * (size_t)sstride * 4, false},
                              {zone_map, (size_t)n_streams * ZN_MAP_WORDS * 4, false},
                              {memo, (size_t)n_streams * (size_t)(max_tracks + 2) * ZN_MEMO_WORDS * 4, true},
                              {zone_ev, (size_t)n_streams * (size_t)max_events * ZN_EV_COLS * 4, true},
                              {zone_count, (size_t)n_streams * 4, true},
                              {zone_occ, (size_t)n_streams * ZN_ZONES * 4, true},
                              {zone_totals, (size_t)n_streams * 2 * ZN_LINES * 4, true}};
        if (regions_clash(reg, (int)(sizeof(reg) / sizeof(reg[0]))))
            return fail(LP_ERR_ARG, fn + "the memo and the four outputs may overlap neither the state, the map nor each other");
    }
    hipLaunchKernelGGL(zone_kernel, dim3((unsigned)n_streams), dim3(ZN_T), 0, (hipStream_t)stream, (const int*)track_state, max_tracks, sstride, nc,
                       (const int*)zone_map, min_hits, memo, zone_ev, zone_count, max_events, zone_occ, zone_totals);
    LP_HIP_CHECK(hipGetLastError());
    return LP_OK;
}
