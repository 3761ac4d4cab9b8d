// tests/cpp/test_stack_scenario.cpp -- mpc_planner_modules/scenario_rows_batch.h (BatchedScenarioRows) through the plain C-ABI, linked once against
// libtmpc_hip.so ("layout": tmpc_scenario_halfspaces / tmpc_scenario_support) and once against the generated libtmpc_hip_safe_horizon.so
// ("columns": setColumns -> tmpc_stack_scenario_halfspaces / tmpc_stack_scenario_support).  One tick: set_batch -> update() (sample, discard,
// halfspaces) -> the parameter rows read back -> tmpc_solve -> support().  The rows, the support counts, the active rows and the empty stages
// are compared with the file tests/test_gpu_cpp_stack_scenario.py wrote from the numpy mirrors, and written out for it.
//   test_stack_scenario <in.bin> <expect.bin> <out.bin> layout|columns
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include <mpc_planner_modules/scenario_rows_batch.h>

static std::vector<double> read_doubles(const char *path)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", path); std::exit(2); }
    std::vector<double> v((size_t)f.tellg() / 8);
    f.seekg(0);
    f.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(v.size() * 8));
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 5) { std::fprintf(stderr, "usage: test_stack_scenario in.bin expect.bin out.bin layout|columns\n"); return 2; }
    const std::vector<double> in = read_doubles(argv[1]), expect = read_doubles(argv[2]);
    const bool columns = std::string(argv[4]) == "columns";
    size_t at = 0;
    auto next = [&]() { if (at >= in.size()) { std::fprintf(stderr, "in.bin is too short\n"); std::exit(2); } return in[at++]; };
    auto take = [&](size_t n) { std::vector<double> v(n); for (auto &x : v) x = next(); return v; };
    const int Q = (int)next(), M = (int)next(), modes = (int)next(), S = (int)next(), n_discard = (int)next(), N = (int)next(), n_rows = (int)next();
    const int B = (int)next(), npar = (int)next();
    const uint64_t seed = (uint64_t)next();
    const double radius = next(), disc_offset = next(), tol = next();
    std::vector<int32_t> cols(1 + 3 * (size_t)n_rows);
    for (auto &c : cols) c = (int32_t)next();
    const std::vector<double> pred = take((size_t)Q * M * modes * N * 6), prob = take((size_t)Q * M * modes), state_x = take(Q);
    std::vector<int> scene_of(B);
    for (auto &s : scene_of) s = (int)next();
    const std::vector<double> xinit = take((size_t)B * 6), x0 = take((size_t)B * (N + 1) * 8), start = take((size_t)B * N * npar);
    if (at != in.size()) { std::fprintf(stderr, "in.bin is too long\n"); return 2; }
    const size_t n_par = (size_t)B * N * npar;
    if (expect.size() != n_par + 3 * (size_t)B) { std::fprintf(stderr, "expect.bin has the wrong size\n"); return 2; }

    tmpc_dims d;
    tmpc_default_dims_ex(&d, N, 5, 0, 0, n_rows, 1);                 // (a generated library answers with its own stack's rows)
    if (d.npar != npar || d.N != N) { std::fprintf(stderr, "the library's shape is %d parameters, N = %d\n", d.npar, d.N); return 1; }
    tmpc_handle *h = nullptr;
    if (tmpc_create_v2(&h, &d, sizeof d, B, 0)) { std::fprintf(stderr, "tmpc_create_v2 failed: %s\n", h ? tmpc_last_error(h) : "no handle"); return 1; }
    auto check = [&](int rc, const char *what) { if (rc) { std::fprintf(stderr, "%s: %s\n", what, tmpc_last_error(h)); std::exit(1); } };
    check(tmpc_set_batch(h, B, xinit.data(), x0.data(), start.data()), "tmpc_set_batch");
    std::vector<double> rows(n_par);
    std::vector<int> support(B), active(B), empty(B);
    {
        MPCPlanner::BatchedScenarioRows scn(h, Q, M, modes, S, n_discard, N, n_rows, B);
        if (columns) scn.setColumns(cols, n_rows);
        scn.update(pred, prob, state_x, scene_of, seed, radius, disc_offset);
        check(tmpc_debug_get_params(h, rows.data()), "tmpc_debug_get_params");
        check(tmpc_solve(h), "tmpc_solve");
        scn.support(tol);
        check(tmpc_synchronize(h), "tmpc_synchronize");
        const size_t bytes = (size_t)B * sizeof(int);
        if (hipMemcpy(support.data(), scn.supports(), bytes, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(active.data(), scn.activeRows(), bytes, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(empty.data(), scn.emptyStages(), bytes, hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "hipMemcpy failed\n"); return 1; }
    }
    tmpc_destroy(h);

    std::vector<double> out(rows);
    for (int b = 0; b < B; b++) out.push_back(support[b]);
    for (int b = 0; b < B; b++) out.push_back(active[b]);
    for (int b = 0; b < B; b++) out.push_back(empty[b]);
    std::ofstream(argv[3], std::ios::binary).write(reinterpret_cast<const char *>(out.data()), (std::streamsize)(out.size() * 8));
    const bool rows_equal = std::memcmp(rows.data(), expect.data(), n_par * 8) == 0;
    bool counts_equal = true;
    int total = 0;
    for (size_t i = n_par; i < out.size(); i++) counts_equal = counts_equal && out[i] == expect[i];
    for (int b = 0; b < B; b++) total += support[b];
    std::printf("[stack scenario cpp] %s: rows bitwise equal to the mirrors' %d, support / active rows / empty stages equal %d, support in all %d\n", argv[4],
                (int)rows_equal, (int)counts_equal, total);
    return rows_equal && counts_equal ? 0 : 1;
}
