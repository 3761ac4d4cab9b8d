// tests/cpp/test_guidance_search.cpp -- MPCPlanner::guidanceSearch (mpc_planner_modules/guidance_search.h) on a case file of
// tests/test_cpp_guidance_search.py: every output and every carried array after every tick, %.17g (a double round-trips), for the comparison
// with mpc_planner_amd/modules.py guidance_search.  Host code only, no GPU.
//   test_guidance_search <case.bin>
// The file is a flat array of doubles: Q n_goals M N ticks n_paths n_samples n_nodes_max max_expansions seed robot_radius max_velocity margin
// weight_length dt, then per tick state4 [Q][4], goals [Q][n_goals][3], obstacle_pos [Q][M][N][2], obstacle_radius [Q][M], selected [Q][M],
// was_reset [Q].  The carried arrays start at zeros, the outputs sentinel-filled once (an unused node keeps the sentinel).
#include <cstdint>
#include <cstdio>
#include <vector>

#include <mpc_planner_modules/guidance_search.h>

template <class T> static void print(const char *name, const std::vector<T> &v)
{
    std::printf("%s", name);
    for (const T &x : v) std::printf(" %.17g", (double)x);
    std::printf("\n");
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<double> in;
    double buf[256];
    size_t got;
    while ((got = std::fread(buf, sizeof(double), 256, f)) > 0) in.insert(in.end(), buf, buf + got);
    std::fclose(f);
    size_t at = 0;
    auto take = [&](size_t n) { std::vector<double> v(in.begin() + at, in.begin() + at + n); at += n; return v; };
    if (in.size() < 15) return 2;
    const std::vector<double> head = take(15);
    const int Q = (int)head[0], G = (int)head[1], M = (int)head[2], N = (int)head[3], ticks = (int)head[4];
    MPCPlanner::GuidanceSearchOptions o{(int)head[5], (int)head[6], (int)head[7], (int)head[8], (unsigned long long)head[9], head[10], head[11], head[12], head[13]};
    const double dt = head[14];
    if (Q <= 0 || G < 0 || G > 64 || M < 0 || M > 64 || N < 1 || N > 64 || ticks < 0) return 2;
    const size_t per_tick = (size_t)Q * (4 + (size_t)G * 3 + (size_t)M * N * 2 + 2 * (size_t)M + 1);
    if (in.size() != 15 + per_tick * (size_t)ticks) return 2;
    auto clamp = [](int v) { return (size_t)(v < 1 ? 1 : (v > 64 ? 64 : v)); };          // (a refused size still gets arrays)
    const size_t P = clamp(o.n_paths), R = clamp(o.n_nodes_max), S = (size_t)N + 1;
    std::vector<double> prev_traj((size_t)Q * P * S * 2, 0.), nodes((size_t)Q * P * R * 3, -3.);
    std::vector<int32_t> prev_class((size_t)Q * P, 0), prev_count(Q, 0), next_class(Q, 0), node_count((size_t)Q * P, -7), traj_count(Q, -7),
        topology_class((size_t)Q * P, -7), status(Q, -7);
    for (int t = 0; t < ticks; t++) {
        const std::vector<double> state4 = take((size_t)Q * 4), goals = take((size_t)Q * G * 3), opos = take((size_t)Q * M * N * 2),
                                  orad = take((size_t)Q * M), seld = take((size_t)Q * M), resetd = take(Q);
        std::vector<int32_t> selected(seld.begin(), seld.end());
        std::vector<uint8_t> was_reset(resetd.begin(), resetd.end());
        if (!MPCPlanner::guidanceSearch(Q, G, M, N, dt, o, state4.data(), goals.data(), opos.data(), orad.data(), selected.data(), was_reset.data(),
                                        prev_traj.data(), prev_class.data(), prev_count.data(), next_class.data(), nodes.data(), node_count.data(),
                                        traj_count.data(), topology_class.data(), status.data())) {
            std::printf("refused\n");
            return 3;
        }
        std::printf("tick %d\n", t);
        print("nodes", nodes); print("node_count", node_count); print("traj_count", traj_count); print("topology_class", topology_class);
        print("status", status); print("prev_traj", prev_traj); print("prev_class", prev_class); print("prev_count", prev_count);
        print("next_class", next_class);
    }
    return 0;
}
