// The column mode of the batched path and free-space twins (mpc_planner_modules/reference_path_batch.h BatchedPathTracking::setColumns,
// mpc_planner_modules/free_space_batch.h BatchedFreeSpace::setColumns) for tests/test_gpu_cpp_stack_env.py: the same program is linked once
// against libtmpc_hip.so and once against the generated libtmpc_hip_road_decomp.so, whose parameter map is the hand-written one of that shape.
//   test_stack_env <config dir> <in.bin> <out.bin> layout     setPaths() -> track() -> setParameters() -> roadHalfspaces() x 2 -> setCostmaps() -> update() ->
//                                                             setParameters() through include/tmpc_hip.h
//   test_stack_env <config dir> <in.bin> <out.bin> columns    the same calls after setColumns(): through include/tmpc_hip_stack_env.h
// and writes to <out.bin> (doubles): the batch's parameter rows (tmpc_debug_get_params) [B][N][npar], the centreline road buffer and the bounds
// road buffer [Q][N][3][3] each, the state buffer [B][nx].
// in.bin (doubles): Q, B, n_seg, n_pcols, n_dcols, size_x, size_y, resolution, range, disc_offset, offset_first, offset_second; pcols; dcols; the
// path: n_seg x (9 coefficients, 8 left, 8 right), length; per scene: x, y, origin_x, origin_y; the costmap [size_y][size_x] (one map, moved per
// scene); scene_of [B]; main_of [Q]; x0 [B][N + 1][nv].
#include <mpc_planner_modules/free_space_batch.h>
#include <mpc_planner_modules/reference_path_batch.h>
#include <mpc_planner_solver/solver_interface.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace MPCPlanner;

template <class T>
static void *upload(const std::vector<T> &v)
{
    void *d = nullptr;
    if (hipMalloc(&d, v.size() * sizeof(T)) != hipSuccess || hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) { std::printf("upload failed\n"); std::exit(1); }
    return d;
}

int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    setSolverConfigPath(argv[1]);
    const bool columns = !std::strcmp(argv[4], "columns");
    FILE *f = std::fopen(argv[2], "rb");
    if (!f) { std::printf("cannot open %s\n", argv[2]); return 2; }
    std::fseek(f, 0, SEEK_END); const long bytes = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    std::vector<double> in(bytes / 8);
    if (std::fread(in.data(), 8, in.size(), f) != in.size()) return 2;
    std::fclose(f);
    size_t o = 0;
    auto next = [&]() { return in.at(o++); };
    const int Q = (int)next(), B = (int)next(), n_seg = (int)next(), n_pcols = (int)next(), n_dcols = (int)next();
    const unsigned int size_x = (unsigned int)next(), size_y = (unsigned int)next();
    const double resolution = next(), range = next(), disc_offset = next(), offset_first = next(), offset_second = next();
    std::vector<int32_t> pcols(n_pcols), dcols(n_dcols);
    for (auto &c : pcols) c = (int32_t)next();
    for (auto &c : dcols) c = (int32_t)next();
    ReferencePathSpline path;
    for (int i = 0; i < n_seg; i++) {
        double r[25];
        for (double &c : r) c = next();
        path.segments.push_back(PathSegment{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8]});
        path.left_bound.push_back(PathSegment{r[9], r[10], r[11], r[12], r[13], r[14], r[15], r[16], r[8]});
        path.right_bound.push_back(PathSegment{r[17], r[18], r[19], r[20], r[21], r[22], r[23], r[24], r[8]});
    }
    path.length = next();
    const int N = SOLVER_N, nx = SOLVER_NX, nv = SOLVER_NX + SOLVER_NU, n_rows = SOLVER_NDECOMP;
    std::vector<double> state((size_t)Q * nx, 0.), origin((size_t)Q * 2);
    for (int q = 0; q < Q; q++) { state[(size_t)q * nx] = next(); state[(size_t)q * nx + 1] = next(); origin[(size_t)q * 2] = next(); origin[(size_t)q * 2 + 1] = next(); }
    std::vector<unsigned char> cost((size_t)size_x * size_y);
    for (auto &c : cost) c = (unsigned char)next();
    std::vector<int> scene_of(B), main_of(Q);
    for (auto &s : scene_of) s = (int)next();
    for (auto &s : main_of) s = (int)next();
    std::vector<double> x0((size_t)B * (N + 1) * nv);
    for (auto &v : x0) v = next();
    if (o != in.size()) { std::printf("input has %zu doubles, %zu read\n", in.size(), o); return 2; }
    std::vector<costmap_2d::Costmap2D> maps;
    for (int q = 0; q < Q; q++) {
        maps.emplace_back(size_x, size_y, resolution, origin[(size_t)q * 2], origin[(size_t)q * 2 + 1]);
        for (unsigned int my = 0; my < size_y; my++)
            for (unsigned int mx = 0; mx < size_x; mx++) maps.back().setCost(mx, my, cost[(size_t)my * size_x + mx]);
    }
    std::vector<const costmap_2d::Costmap2D *> map_of;
    for (auto &m : maps) map_of.push_back(&m);

    tmpc_dims d;
    tmpc_default_dims_ex(&d, SOLVER_N, SOLVER_S, SOLVER_NLIN, SOLVER_M, SOLVER_NSLK, SOLVER_SLACK);     // a generated library fixes the row structure itself
    if (d.npar != SOLVER_NP) { std::printf("npar %d, expected %d\n", d.npar, SOLVER_NP); return 1; }
    tmpc_handle *h = nullptr;
    if (tmpc_create(&h, &d, B, 0)) { std::printf("tmpc_create failed\n"); return 1; }
    std::vector<double> xinit((size_t)B * nx, 0.), rows((size_t)B * N * SOLVER_NP, -7.);
    if (tmpc_set_batch(h, B, xinit.data(), x0.data(), rows.data())) { std::printf("%s\n", tmpc_last_error(h)); return 1; }
    std::vector<double> state_x(Q), road((size_t)Q * N * 3 * 3, -5.), stateB((size_t)B * nx, -9.), road_centre(road.size()), road_bounds(road.size());
    for (int q = 0; q < Q; q++) state_x[q] = state[(size_t)q * nx];
    void *d_state = upload(state), *d_state_x = upload(state_x), *d_main = upload(main_of), *d_road_centre = upload(road), *d_road_bounds = upload(road), *d_stateB = upload(stateB);
    {
        BatchedPathTracking tracking(h, Q, n_seg + 3, SOLVER_S, true);
        BatchedFreeSpace free_space(h, Q, (int)size_x, (int)size_y, 4096, N, range, n_rows);
        if (columns) { tracking.setColumns(pcols); free_space.setColumns(dcols); }
        tracking.setPaths(std::vector<ReferencePathSpline>((size_t)Q, path));
        tracking.track(d_state, nx);
        tracking.setParameters(scene_of, d_stateB);
        tracking.roadHalfspaces(d_main, offset_first, offset_second, d_road_centre, 3, 1);
        tracking.roadHalfspaces(d_main, 0.325, 0.325, d_road_bounds, 3, 0, true);
        free_space.setCostmaps(map_of);
        free_space.update(d_main, n_seg + 3, tracking.paths(), tracking.pathCounts(), tracking.pathLengths(), tracking.closestS(), d_state_x);
        free_space.setParameters(scene_of, disc_offset);
        if (tmpc_synchronize(h) || tmpc_debug_get_params(h, rows.data())) { std::printf("%s\n", tmpc_last_error(h)); return 1; }
        if (hipMemcpy(road_centre.data(), d_road_centre, road.size() * 8, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(road_bounds.data(), d_road_bounds, road.size() * 8, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(stateB.data(), d_stateB, stateB.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return 1;
    }
    for (void *p : {d_state, d_state_x, d_main, d_road_centre, d_road_bounds, d_stateB}) (void)hipFree(p);
    tmpc_destroy(h);
    FILE *g = std::fopen(argv[3], "wb");
    if (!g) return 2;
    for (const std::vector<double> *v : {&rows, &road_centre, &road_bounds, &stateB})
        if (std::fwrite(v->data(), 8, v->size(), g) != v->size()) return 2;
    std::fclose(g);
    std::printf("rows %s entries %d stages %d npar %d\n", columns ? "columns" : "layout", B, N, SOLVER_NP);
    return 0;
}
