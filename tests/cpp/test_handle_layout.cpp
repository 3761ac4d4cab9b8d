// The handle's I/O table (mpc_planner_amd/csrc/tmpc_handle_layout.hpp) on the host alone: alignment, order and disjointness of the regions, the totals, and
// the sizes at which a handle stops being tick-size (tests/test_cpp_handle_layout.py builds and runs it).
#include <cstdio>
#include <initializer_list>
#include "tmpc_handle_layout.hpp"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; std::printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static size_t up256(size_t x) { return (x + 255) / 256 * 256; }

// one allocation: offsets multiples of 256, regions disjoint and in table order, the total = the last offset + its rounded size
static void check_regions(const tmpc::IoRegion *r, int n, size_t total, size_t B_max, const char *what)
{
    for (int i = 0; i < n; i++) {
        CHECK(r[i].per_traj > 0, "%s[%d]", what, i);
        CHECK(r[i].offset % 256 == 0, "%s[%d] offset %zu", what, i, r[i].offset);
        CHECK(r[i].bytes(B_max) == B_max * r[i].per_traj, "%s[%d]", what, i);
        if (i > 0) CHECK(r[i].offset >= r[i - 1].offset + r[i - 1].bytes(B_max), "%s[%d] at %zu overlaps [%d] (%zu + %zu)", what, i, r[i].offset, i - 1,
                         r[i - 1].offset, r[i - 1].bytes(B_max));
        if (i > 0) CHECK(r[i].offset == r[i - 1].offset + up256(r[i - 1].bytes(B_max)), "%s[%d] not packed", what, i);
    }
    CHECK(r[0].offset == 0, "%s", what);
    CHECK(total == r[n - 1].offset + up256(r[n - 1].bytes(B_max)), "%s total %zu", what, total);
}

static tmpc::IoLayout checked(size_t N, size_t nxe, size_t nve, size_t npar, size_t B_max)
{
    const tmpc::IoLayout l = tmpc::io_layout(N, nxe, nve, npar, B_max);
    check_regions(l.in, tmpc::IN_COUNT, l.in_total, B_max, "in");
    check_regions(l.out, tmpc::OUT_COUNT, l.out_total, B_max, "out");
    CHECK(l.tick == (l.in_total <= (2u << 20) && l.out_total <= (2u << 20)), "B_max %zu", B_max);
    // bytes per trajectory, from the arrays' shapes (include/tmpc_hip.h): doubles but for the four i32 outputs and the i32 slot map
    const size_t in_per[tmpc::IN_COUNT] = {nxe * 8, (N + 1) * nve * 8, N * npar * 8, 4};
    const size_t out_per[tmpc::OUT_COUNT] = {(N + 1) * nxe * 8, N * 2 * 8, 8, 8, 4, 4, 4, 4};
    for (int i = 0; i < tmpc::IN_COUNT; i++) CHECK(l.in[i].per_traj == in_per[i], "in[%d] %zu", i, l.in[i].per_traj);
    for (int i = 0; i < tmpc::OUT_COUNT; i++) CHECK(l.out[i].per_traj == out_per[i], "out[%d] %zu", i, l.out[i].per_traj);
    for (size_t B : {(size_t)1, B_max}) CHECK(l.batch_bytes(B) == B * (in_per[0] + in_per[1] + in_per[2]), "batch_bytes(%zu)", B);
    return l;
}

int main()
{
    // the properties: odd sizes, one trajectory, slack shapes (ext_nx 6, ext_nv 8), the horizon's bounds, the bench's handle
    const size_t shapes[][4] = {{20, 5, 7, 135}, {20, 5, 7, 39}, {30, 5, 7, 135}, {2, 5, 7, 11}, {62, 6, 8, 307}, {21, 6, 8, 77}};
    for (const auto &s : shapes)
        for (size_t B : {1, 2, 5, 8, 63, 64, 65, 91, 92, 255, 256, 257, 272, 281, 282, 4096, 32768}) checked(s[0], s[1], s[2], s[3], B);

    // cfg 2 (N = 20, ext_nx 5, ext_nv 7, npar 135): 91 trajectories are the largest tick-size handle
    tmpc::IoLayout l = checked(20, 5, 7, 135, 91);
    CHECK(l.in_total == 2077440 && l.tick, "in_total %zu tick %d", l.in_total, (int)l.tick);
    l = checked(20, 5, 7, 135, 92);
    CHECK(l.in_total == 2099968 && !l.tick, "in_total %zu tick %d", l.in_total, (int)l.tick);
    l = checked(20, 5, 7, 135, 64);
    CHECK(l.batch_bytes(22) == 22 * 22816 && l.batch_bytes(22) <= (512u << 10) && l.batch_bytes(23) > (512u << 10), "batch_bytes(22) %zu", l.batch_bytes(22));
    CHECK(l.out_total <= (256u << 10) && l.in[tmpc::IN_PARAMS].offset <= (256u << 10), "cfg 2 at 64: %zu %zu", l.out_total, l.in[tmpc::IN_PARAMS].offset);
    // N = 20, npar 39: tick-size up to 281 trajectories; at 272 the params region starts beyond 256 KiB and the outputs exceed 256 KiB
    l = checked(20, 5, 7, 39, 272);
    CHECK(l.in_total == 2029568 && l.out_total == 325376 && l.tick, "in_total %zu out_total %zu tick %d", l.in_total, l.out_total, (int)l.tick);
    CHECK(l.in[tmpc::IN_PARAMS].offset == 331008, "params at %zu", l.in[tmpc::IN_PARAMS].offset);
    CHECK(l.batch_bytes(70) == 70 * 7456 && l.batch_bytes(70) <= (512u << 10) && l.batch_bytes(71) > (512u << 10), "batch_bytes(70) %zu", l.batch_bytes(70));
    CHECK(checked(20, 5, 7, 39, 281).tick, "281");
    CHECK(!checked(20, 5, 7, 39, 282).tick, "282");

    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("handle layout ok\n");
    return 0;
}
