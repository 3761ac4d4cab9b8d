// The Solver-free free-space header (mpc_planner_modules/free_space.h, mpc_planner_types/costmap.h) as a stand-alone program, for
// tests/test_cpp_free_space.py: reads launches written by the test as a file of doubles and prints what the header computes with %.17g, which
// round-trips a double, so the test can compare bit for bit against the numpy mirror.
//   decomp <file>    Q N n_pts_max n_rows n_seg range dt, then per scene: segments (n_seg) rows [n_seg][9] length s0 state_x v[N] count points[n_pts_max][2]
//   costmap <file>   size_x size_y origin_x origin_y resolution max_points, then the costs [size_y][size_x]
// With -DWITH_SOLVER, against a generated solver's headers (slack model, 12 decomp rows):
//   module <config dir> <scene.bin>   CPU: DecompConstraints::isDataReady / update / setParameters on one scene; prints the written parameters
//   batch <config dir> <scene.bin>    needs a GPU: BatchedFreeSpace's two ticks against FreeSpace::decomposePath on the host, bitwise
//   scene.bin: n_rows range n_seg, rows [n_seg][9], length, x y spline, v[N] (tick 1) v[N] (tick 2), disc_offset, size_x size_y origin_x origin_y
//   resolution, the costs [size_y][size_x]
#include <cstdio>
#include <string>
#include <vector>

#ifdef WITH_SOLVER
#include <cstring>
#include <mpc_planner_modules/modules_hip.h>
#include <mpc_planner_modules/free_space_batch.h>
#else
#include <mpc_planner_modules/free_space.h>
#include <mpc_planner_types/costmap.h>
#endif

using namespace MPCPlanner;

static std::vector<double> read_all(const char *file)
{
    std::vector<double> v;
    FILE *f = std::fopen(file, "rb");
    if (!f) return v;
    double x;
    while (std::fread(&x, sizeof(double), 1, f) == 1) v.push_back(x);
    std::fclose(f);
    return v;
}

static int decomp(const std::vector<double> &in)
{
    size_t o = 0;
    auto next = [&]() { return in.at(o++); };
    const int Q = (int)next(), N = (int)next(), n_pts_max = (int)next(), n_rows = (int)next(), n_seg = (int)next();
    const double range = next(), dt = next();
    for (int q = 0; q < Q; q++) {
        ReferencePathSpline path;
        const int segments = (int)next();
        for (int i = 0; i < n_seg; i++) {
            double r[9];
            for (double &c : r) c = next();
            if (i < segments) path.segments.push_back(PathSegment{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8]});
        }
        path.length = next();
        const double s0 = next(), state_x = next();
        std::vector<double> v(N);
        for (double &c : v) c = next();
        int count = (int)next();
        count = count < 0 ? 0 : (count > n_pts_max ? n_pts_max : count);
        std::vector<double> points(in.begin() + o, in.begin() + o + 2 * (size_t)count);
        o += 2 * (size_t)n_pts_max;
        std::vector<double> rows;
        std::vector<int> written, status;
        FreeSpace::decomposePath(path, s0, v, dt, points, range, n_rows, state_x, rows, written, status);
        for (int k = 0; k < N; k++) {
            std::printf("stage %d %d %d %d\n", q, k, written[k], status[k]);
            for (int r = 0; r < n_rows; r++) {
                const double *row = &rows[((size_t)k * n_rows + r) * 3];
                std::printf("row %d %d %d %.17g %.17g %.17g\n", q, k, r, row[0], row[1], row[2]);
            }
        }
    }
    return o == in.size() ? 0 : 3;
}

static int costmap(const std::vector<double> &in)
{
    size_t o = 0;
    auto next = [&]() { return in.at(o++); };
    const unsigned int size_x = (unsigned int)next(), size_y = (unsigned int)next();
    const double origin_x = next(), origin_y = next(), resolution = next();
    const size_t max_points = (size_t)next();
    costmap_2d::Costmap2D map(size_x, size_y, resolution, origin_x, origin_y);
    for (unsigned int my = 0; my < size_y; my++)
        for (unsigned int mx = 0; mx < size_x; mx++) map.setCost(mx, my, (unsigned char)next());
    std::vector<double> xy;
    const bool overflow = FreeSpace::occupiedCells(map, xy, max_points);
    std::printf("points %zu %d\n", xy.size() / 2, (int)overflow);
    for (size_t i = 0; i + 1 < xy.size(); i += 2) std::printf("p %.17g %.17g\n", xy[i], xy[i + 1]);
    return o == in.size() ? 0 : 3;
}

#ifdef WITH_SOLVER
struct Scene
{
    int n_rows; double range; ReferencePathSpline path; double x, y, spline; std::vector<double> v[2]; double disc_offset;
    costmap_2d::Costmap2D map;
};
static Scene read_scene(const std::vector<double> &in)
{
    size_t o = 0;
    auto next = [&]() { return in.at(o++); };
    Scene sc;
    sc.n_rows = (int)next(); sc.range = next();
    const int n_seg = (int)next();
    for (int i = 0; i < n_seg; i++) {
        double r[9];
        for (double &c : r) c = next();
        sc.path.segments.push_back(PathSegment{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8]});
    }
    sc.path.length = next();
    sc.x = next(); sc.y = next(); sc.spline = next();
    for (auto &v : sc.v) { v.resize(SOLVER_N); for (double &c : v) c = next(); }
    sc.disc_offset = next();
    const unsigned int size_x = (unsigned int)next(), size_y = (unsigned int)next();
    const double origin_x = next(), origin_y = next(), resolution = next();
    sc.map = costmap_2d::Costmap2D(size_x, size_y, resolution, origin_x, origin_y);
    for (unsigned int my = 0; my < size_y; my++)
        for (unsigned int mx = 0; mx < size_x; mx++) sc.map.setCost(mx, my, (unsigned char)next());
    return sc;
}

static int module(Scene &sc)
{
    ModuleConfig cfg;
    cfg.decomp_range = sc.range; cfg.decomp_max_constraints = sc.n_rows;
    auto solver = std::make_shared<Solver>();
    for (int k = 0; k < solver->N; k++) solver->setEgoPrediction(k, "v", sc.v[0][k]);
    State state;
    state.set("x", sc.x); state.set("y", sc.y); state.set("spline", sc.spline);
    RealTimeData data;
    data.robot_area.emplace_back(sc.disc_offset, 0.325);
    data.reference_path = sc.path.segments; data.reference_path_length = sc.path.length;
    ModuleData module_data;
    DecompConstraints decomp(solver, cfg);
    std::string missing;
    const bool ready_without = decomp.isDataReady(data, missing);
    data.costmap = &sc.map;
    std::string none;
    std::printf("ready %d [%s] %d [%s]\n", (int)ready_without, missing.c_str(), (int)decomp.isDataReady(data, none), none.c_str());
    decomp.update(state, data, module_data);
    std::printf("points %zu exceeded %d\n", decomp.occupiedPositions().size() / 2, (int)decomp.exceeded());
    for (int k = 0; k < solver->N; k++) {
        decomp.setParameters(data, module_data, k);
        std::printf("stage %d %d %d %.17g\n", k, decomp.rowCounts()[k], decomp.status()[k], solver->getParameter(k, "ego_disc_0_offset"));
        for (int j = 0; j < SOLVER_NDECOMP; j++) {
            const std::string name = "disc_0_decomp_" + std::to_string(j);
            std::printf("row %d %d %.17g %.17g %.17g\n", k, j, solver->getParameter(k, name + "_a1"), solver->getParameter(k, name + "_a2"), solver->getParameter(k, name + "_b"));
        }
    }
    return 0;
}

template <class T>
static void *upload(const std::vector<T> &v)
{
    void *d = nullptr;
    if (hipMalloc(&d, v.size() * sizeof(T)) != hipSuccess || hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) { std::printf("upload failed\n"); std::exit(1); }
    return d;
}

// two scenes: the scene's map, and the same map moved by (0.3, -0.2); two ticks: the second with other speeds and the maps unchanged (no second
// extraction of the points); after each tick the twin's rows, counts and statuses against FreeSpace::decomposePath, and after the second the
// written parameters against the rows
static int batch(Scene &sc)
{
    const int Q = 2, B = 3, N = SOLVER_N, n_rows = sc.n_rows, R = sc.path.numSegments() + 3, nv = SOLVER_NX + SOLVER_NU;
    costmap_2d::Costmap2D moved(sc.map.getSizeInCellsX(), sc.map.getSizeInCellsY(), sc.map.getResolution(), sc.map.getOriginX() + 0.3, sc.map.getOriginY() - 0.2);
    for (unsigned int my = 0; my < sc.map.getSizeInCellsY(); my++)
        for (unsigned int mx = 0; mx < sc.map.getSizeInCellsX(); mx++) moved.setCost(mx, my, sc.map.getCost(mx, my));
    const costmap_2d::Costmap2D *maps[Q] = {&sc.map, &moved};
    tmpc_dims d;
    tmpc_default_dims_ex(&d, SOLVER_N, SOLVER_S, SOLVER_NLIN, SOLVER_M, SOLVER_NSLK, SOLVER_SLACK);
    tmpc_handle *h = nullptr;
    if (tmpc_create(&h, &d, B, 0)) { std::printf("tmpc_create failed\n"); return 1; }
    std::vector<double> path((size_t)Q * R * 9, -3.0), length(Q, sc.path.length), s0 = {sc.spline, sc.spline + 0.25}, state_x = {sc.x, sc.x + 1.0};
    std::vector<int> count(Q, sc.path.numSegments()), main_of = {0, 2};     // entry 1 belongs to scene 0 too
    for (int q = 0; q < Q; q++)
        for (int i = 0; i < sc.path.numSegments(); i++) { coefficients(sc.path.segments[i], &path[((size_t)q * R + i) * 9]); path[((size_t)q * R + i) * 9 + 8] = sc.path.segments[i].start; }
    void *d_path = upload(path), *d_length = upload(length), *d_s0 = upload(s0), *d_state_x = upload(state_x), *d_count = upload(count), *d_main = upload(main_of);
    size_t differ = 0, params_differ = 0;
    int points[Q] = {0, 0};
    {
        BatchedFreeSpace twin(h, Q, (int)sc.map.getSizeInCellsX(), (int)sc.map.getSizeInCellsY(), 4096, N, sc.range, n_rows);
        twin.setCostmaps({maps[0], maps[1]});
        std::vector<double> xinit((size_t)B * SOLVER_NX, 0.), x0((size_t)B * (N + 1) * nv, 0.), params((size_t)B * N * SOLVER_NP, -3.0), got(params.size());
        for (int tick = 0; tick < 2; tick++) {
            for (int b = 0; b < B; b++)
                for (int k = 0; k < N; k++) x0[((size_t)b * (N + 1) + k) * nv + 5] = sc.v[b == 2 ? 1 - tick : tick][k];      // column 5: v
            if (tmpc_set_batch(h, B, xinit.data(), x0.data(), params.data())) { std::printf("tmpc_set_batch: %s\n", tmpc_last_error(h)); return 1; }
            twin.update(d_main, R, d_path, d_count, d_length, d_s0, d_state_x);
            twin.setParameters({0, 0, 1}, sc.disc_offset);
            if (tmpc_synchronize(h) || tmpc_debug_get_params(h, got.data())) { std::printf("%s\n", tmpc_last_error(h)); return 1; }
            std::vector<double> rows((size_t)Q * N * n_rows * 3);
            std::vector<int> rc((size_t)Q * N), np(Q);
            std::vector<unsigned char> st((size_t)Q * N);
            if (hipMemcpy(rows.data(), twin.rows(), rows.size() * 8, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(rc.data(), twin.rowCounts(), rc.size() * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(st.data(), twin.status(), st.size(), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(np.data(), twin.pointCounts(), Q * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return 1;
            for (int q = 0; q < Q; q++) {
                std::vector<double> occ, want;
                std::vector<int> wc, ws;
                FreeSpace::occupiedCells(*maps[q], occ, 4096);
                FreeSpace::decomposePath(sc.path, s0[q], sc.v[q == 1 ? 1 - tick : tick], SOLVER_DT, occ, sc.range, n_rows, state_x[q], want, wc, ws);
                points[q] = np[q];
                differ += (size_t)np[q] != occ.size() / 2;
                differ += std::memcmp(&rows[(size_t)q * N * n_rows * 3], want.data(), want.size() * 8) != 0;
                for (int k = 0; k < N; k++) differ += rc[(size_t)q * N + k] != wc[k] || st[(size_t)q * N + k] != ws[k];
            }
            // the written parameters: entries 0 and 1 carry scene 0's rows, entry 2 scene 1's; every other column keeps the prefill
            Solver names;
            for (int b = 0; b < B; b++)
                for (int k = 0; k < N; k++) {
                    const double *p = &got[((size_t)b * N + k) * SOLVER_NP];
                    std::vector<char> touched(SOLVER_NP, 0);
                    const int off = names._parameter_map.at("ego_disc_0_offset");
                    touched[off] = 1; params_differ += p[off] != sc.disc_offset;
                    for (int j = 0; j < n_rows; j++)
                        for (int c = 0; c < 3; c++) {
                            const int idx = names._parameter_map.at("disc_0_decomp_" + std::to_string(j) + (c == 0 ? "_a1" : c == 1 ? "_a2" : "_b"));
                            touched[idx] = 1;
                            params_differ += std::memcmp(&p[idx], &rows[((((size_t)(b == 2 ? 1 : 0)) * N + k) * n_rows + j) * 3 + c], 8) != 0;
                        }
                    for (int i = 0; i < SOLVER_NP; i++) params_differ += !touched[i] && p[i] != -3.0;
                }
        }
    }
    std::printf("batch differ %zu params_differ %zu points %d %d\n", differ, params_differ, points[0], points[1]);
    for (void *p : {d_path, d_length, d_s0, d_state_x, d_count, d_main}) (void)hipFree(p);
    tmpc_destroy(h);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    setSolverConfigPath(argv[2]);
    const std::vector<double> in = read_all(argv[3]);
    if (in.empty()) return 2;
    Scene sc = read_scene(in);
    return std::string(argv[1]) == "batch" ? batch(sc) : module(sc);
}
#else
int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::vector<double> in = read_all(argv[2]);
    if (in.empty()) return 2;
    return std::string(argv[1]) == "costmap" ? costmap(in) : decomp(in);
}
#endif
