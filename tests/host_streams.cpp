// Stand-alone host program for yolo-lp_amd/csrc/lp_streams.h (tests/test_streams_cpu.py builds and runs it; no GPU, no HIP).
// The planner is checked against its stated properties, written here without looking at how it computes them: each tracked frame's
// workgroup carries the frame's stream, workgroups are numbered by first appearance, one per distinct stream of the launch, the
// untracked frames follow the policy, the rest of the table is zero and the scratch vector comes back all -1.
#include "../yolo-lp_amd/csrc/lp_streams.h"

#include <cstdio>

using namespace lp;

static int failures = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            ++failures;                                      \
            std::printf("FAILED %s:%d: %s | ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                        \
            std::printf("\n");                               \
        }                                                    \
    } while (0)

constexpr int N_STREAMS = 66, FR = LP_FRAMES_PER_LAUNCH;

static void check_launch(const char* name, const int* so, int nf, int b0, Untracked policy, std::vector<int>& blk_of) {
    const StreamPlan pl = plan_streams(so, nf, blk_of, policy);
    const char* pol = policy == UNTRACKED_DEAL ? "deal" : "leave out";
    // the distinct streams of the launch in order of first appearance
    std::vector<int> order;
    for (int j = 0; j < nf; ++j) {
        bool seen = so[j] < 0;
        for (int s : order) seen = seen || s == so[j];
        if (!seen) order.push_back(so[j]);
    }
    const int D = (int)order.size();
    if (D > 0) CHECK(pl.nblk == D, "%s, %s, frame %d: %d workgroups for %d streams", name, pol, b0, pl.nblk, D);
    else if (policy == UNTRACKED_DEAL) CHECK(pl.nblk == 1 && pl.blk_stream[0] == -1, "%s, %s, frame %d: nblk %d, stream %d", name, pol, b0, pl.nblk, pl.blk_stream[0]);
    else CHECK(pl.nblk == 0, "%s, %s, frame %d: nblk %d", name, pol, b0, pl.nblk);
    CHECK(pl.nblk <= FR && (policy != UNTRACKED_DEAL || pl.nblk >= 1), "%s, %s, frame %d: nblk %d", name, pol, b0, pl.nblk);
    if (pl.nblk > FR) return;
    for (int k = 0; k < D && k < pl.nblk; ++k)
        CHECK(pl.blk_stream[k] == order[(size_t)k], "%s, %s, frame %d: workgroup %d has stream %d, want %d", name, pol, b0, k, pl.blk_stream[k], order[(size_t)k]);
    for (int j = 0; j < nf; ++j) {
        const int blk = pl.fr_blk[j];
        if (so[j] >= 0) {
            CHECK(blk >= 0 && blk < pl.nblk && pl.blk_stream[blk] == so[j] && pl.fr_skip[j] == 0, "%s, %s, frame %d: workgroup %d, skip %d", name, pol,
                  b0 + j, blk, pl.fr_skip[j]);
        } else if (policy == UNTRACKED_DEAL) {
            CHECK(pl.fr_skip[j] == 1 && blk == j % pl.nblk, "%s, %s, frame %d: workgroup %d of %d, skip %d", name, pol, b0 + j, blk, pl.nblk, pl.fr_skip[j]);
        } else {
            CHECK(blk == -1, "%s, %s, frame %d: workgroup %d", name, pol, b0 + j, blk);
        }
    }
    // what no frame and no workgroup uses stays zero, as in a table that starts zeroed
    for (int k = pl.nblk; k < FR; ++k) CHECK(pl.blk_stream[k] == 0, "%s, %s, frame %d: blk_stream[%d] = %d", name, pol, b0, k, pl.blk_stream[k]);
    for (int j = nf; j < FR; ++j) CHECK(pl.fr_blk[j] == 0 && pl.fr_skip[j] == 0, "%s, %s, frame %d: entry %d behind the launch", name, pol, b0, j);
    for (int s = 0; s < N_STREAMS; ++s) CHECK(blk_of[(size_t)s] == -1, "%s, %s, frame %d: blk_of[%d] = %d on return", name, pol, b0, s, blk_of[(size_t)s]);
}

static void check_list(const char* name, const std::vector<int>& so) {
    CHECK(stream_of_fault(so.data(), (int)so.size(), N_STREAMS).empty(), "%s", name);
    for (Untracked policy : {UNTRACKED_DEAL, UNTRACKED_LEAVE_OUT}) {
        std::vector<int> blk_of((size_t)N_STREAMS, -1);
        const int B = (int)so.size();
        int b0 = 0;
        do {                                                            // the launches of a call (an empty list: one of no frames)
            check_launch(name, so.data() + b0, B - b0 < FR ? B - b0 : FR, b0, policy, blk_of);
            b0 += FR;
        } while (b0 < B);
    }
}

static void check_planner() {
    std::vector<int> v;
    check_list("empty", v);
    check_list("[0]", {0});
    v.clear();
    for (int j = 0; j < 64; ++j) v.push_back(63 - j);
    check_list("64 distinct", v);
    check_list("65 of one stream", std::vector<int>(65, 5));
    v.clear();
    for (int j = 0; j < 66; ++j) v.push_back((j * 5) % 66);              // a permutation of 0..65
    check_list("66 distinct", v);
    v.clear();
    for (int j = 0; j < 130; ++j) v.push_back(j % 3 == 2 ? -1 : (j % 2 ? 7 : 40));
    check_list("130 alternating", v);
    check_list("70 untracked", std::vector<int>(70, -1));
    v.assign(64, -1);
    v.push_back(1);
    v.push_back(0);
    check_list("64 untracked + [1, 0]", v);
}

static void check_rules() {
    const int lo[] = {0, -2, 3}, hi[] = {0, 1, N_STREAMS}, fine[] = {-1, N_STREAMS - 1, 0};
    CHECK(stream_of_fault(lo, 3, N_STREAMS) == "stream -2 of frame 1 (need -1 or 0..65)", "%s", stream_of_fault(lo, 3, N_STREAMS).c_str());
    CHECK(stream_of_fault(hi, 3, N_STREAMS) == "stream 66 of frame 2 (need -1 or 0..65)", "%s", stream_of_fault(hi, 3, N_STREAMS).c_str());
    CHECK(stream_of_fault(fine, 3, N_STREAMS).empty() && stream_of_fault(nullptr, 0, N_STREAMS).empty(), "accepted values");
    CHECK(stream_dims_fault(1, 1).empty() && stream_dims_fault(7, LP_TRACK_MAX_TRACKS).empty(), "accepted dimensions");
    const int bad[][2] = {{0, 4}, {1, 0}, {1, LP_TRACK_MAX_TRACKS + 1}, {-1, -1}};
    for (const auto& d : bad) CHECK(stream_dims_fault(d[0], d[1]) == "need n_streams >= 1 and max_tracks in 1..128", "(%d, %d)", d[0], d[1]);
}

static void check_regions() {
    static char buf[64];
    CHECK(!overlap(buf, 16, buf + 16, 16) && !overlap(buf + 16, 16, buf, 16), "adjacent");
    CHECK(overlap(buf, 16, buf + 15, 16) && overlap(buf + 15, 16, buf, 16), "one byte");
    CHECK(!overlap(buf, 16, buf + 4, 0) && !overlap(buf + 4, 0, buf, 16) && !overlap(buf, 0, buf, 0), "zero length");
    for (int first_out = 0; first_out < 2; ++first_out) {
        const Region adjacent[] = {{buf, 16, first_out != 0}, {buf + 16, 16, first_out == 0}, {buf + 32, 32, true}};
        CHECK(!regions_clash(adjacent, 3), "adjacent buffers, output %d", first_out);
        const Region a[] = {{buf, 16, first_out != 0}, {buf + 15, 16, first_out == 0}}, b[] = {a[1], a[0]};
        CHECK(regions_clash(a, 2) && regions_clash(b, 2), "one byte of overlap, output %d", first_out);
    }
    const Region both_out[] = {{buf, 16, true}, {buf + 40, 8, false}, {buf + 15, 16, true}};
    CHECK(regions_clash(both_out, 3), "two outputs");
    const Region inputs[] = {{buf, 32, false}, {buf + 8, 32, false}, {buf + 40, 8, true}};
    CHECK(!regions_clash(inputs, 3), "inputs may overlap each other");
    const Region empty[] = {{buf, 32, false}, {buf + 8, 0, true}, {nullptr, 0, true}, {buf + 32, 8, true}};
    CHECK(!regions_clash(empty, 4) && !regions_clash(empty, 0), "a region of no bytes overlaps nothing");
}

static void check_thresholds() {
    for (double t : {0.0, 0.3, 0.45, 0.5, 1.0, 0.1 + 1e-12, 3.0e38, 1e-46, -0.25}) {
        const float a = f32_not_above(t), b = f32_not_below(t);
        CHECK((double)a <= t && (double)nextafterf(a, INFINITY) > t, "f32_not_above(%.17g) = %.9g", t, (double)a);
        CHECK((double)b >= t && (double)nextafterf(b, -INFINITY) < t, "f32_not_below(%.17g) = %.9g", t, (double)b);
    }
}

int main() {
    check_planner();
    check_rules();
    check_regions();
    check_thresholds();
    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("all checks passed\n");
    return failures ? 1 : 0;
}
