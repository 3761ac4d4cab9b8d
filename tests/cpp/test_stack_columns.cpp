// The column mode of the batched obstacle twin (mpc_planner/data_preparation_batch.h, BatchedObstaclePreparation::setColumns) for tests/test_gpu_cpp_stack_columns.py:
// the same program is linked once against libtmpc_hip.so and once against the generated libtmpc_hip_tmpc_cfg2.so, whose parameter map is the hand-written one.
//   test_stack_columns <config dir> <in.bin> <out.bin> layout     prepare() -> setParameters() -> linearizeTopology() through include/tmpc_hip.h
//   test_stack_columns <config dir> <in.bin> <out.bin> columns    the same three calls after setColumns(): through include/tmpc_hip_stack.h
// and writes the batch's parameter rows (tmpc_debug_get_params) to <out.bin>.  Constant-velocity mode, probabilistic, two uncertainty passes.
// in.bin (doubles): Q, n, B, n_ocols, n_tcols; ocols; tcols; per scene: x y psi v, count, n x (x y vx vy radius); scene_of [B]; is_original [B];
// x0 [B][N + 1][7].
#include <mpc_planner/data_preparation_batch.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace MPCPlanner;

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
    auto next = [&]() { return in[o++]; };
    const int Q = (int)next(), n = (int)next(), B = (int)next(), n_ocols = (int)next(), n_tcols = (int)next();
    std::vector<int32_t> ocols(n_ocols), tcols(n_tcols);
    for (auto &c : ocols) c = (int32_t)next();
    for (auto &c : tcols) c = (int32_t)next();
    ModuleConfig cfg;
    cfg.max_obstacles = SOLVER_MAX_OBSTACLES;
    cfg.probabilistic_enable = true;
    const int N = cfg.N;
    std::vector<State> states(Q);
    std::vector<std::vector<DynamicObstacle>> lists(Q);
    std::vector<std::vector<Vector2d>> vels(Q);
    const char *sn[] = {"x", "y", "psi", "v"};
    for (int q = 0; q < Q; q++) {
        for (int i = 0; i < 4; i++) states[q].set(sn[i], next());
        const int count = (int)next();
        for (int i = 0; i < n; i++) {
            const double x = next(), y = next(), vx = next(), vy = next(), r = next();
            if (i >= count) continue;
            lists[q].emplace_back(i, Vector2d(x, y), 0., r);
            vels[q].emplace_back(vx, vy);
        }
    }
    std::vector<int> scene_of(B);
    for (auto &s : scene_of) s = (int)next();
    std::vector<uint8_t> is_original(B);
    for (auto &s : is_original) s = (uint8_t)next();
    std::vector<double> x0((size_t)B * (N + 1) * (SOLVER_NX + SOLVER_NU));
    for (auto &v : x0) v = next();
    if (o != in.size()) { std::printf("input has %zu doubles, %zu read\n", in.size(), o); return 2; }

    tmpc_dims d;
    tmpc_default_dims_ex(&d, SOLVER_N, SOLVER_S, SOLVER_NLIN, SOLVER_M, SOLVER_NSLK, SOLVER_SLACK);     // a generated library fixes the row structure itself
    if (d.npar != SOLVER_NP) { std::printf("npar %d, expected %d\n", d.npar, SOLVER_NP); return 1; }
    tmpc_handle *h = nullptr;
    if (tmpc_create(&h, &d, B, 0)) { std::printf("tmpc_create failed\n"); return 1; }
    std::vector<double> xinit((size_t)B * SOLVER_NX, 0.), rows((size_t)B * N * SOLVER_NP, -7.);
    if (tmpc_set_batch(h, B, xinit.data(), x0.data(), rows.data())) { std::printf("%s\n", tmpc_last_error(h)); return 1; }
    void *d_is_original = nullptr;
    if (hipMalloc(&d_is_original, B) != hipSuccess || hipMemcpy(d_is_original, is_original.data(), B, hipMemcpyHostToDevice) != hipSuccess) return 1;
    {
        BatchedObstaclePreparation twin(h, Q, n, cfg);
        if (columns) twin.setColumns(0, ocols, tcols);
        twin.prepare(lists, states, &vels, 2);
        twin.setParameters(scene_of, 0.03);
        twin.linearizeTopology(scene_of, d_is_original);
        if (tmpc_debug_get_params(h, rows.data())) { std::printf("%s\n", tmpc_last_error(h)); return 1; }
    }
    (void)hipFree(d_is_original);
    tmpc_destroy(h);
    FILE *g = std::fopen(argv[3], "wb");
    if (!g || std::fwrite(rows.data(), 8, rows.size(), g) != rows.size()) return 2;
    std::fclose(g);
    std::printf("rows %s entries %d stages %d npar %d\n", columns ? "columns" : "layout", B, N, SOLVER_NP);
    return 0;
}
